// Tucker3 / RESCAL scorer with a projected relation (LookupTucker3RelationModel: openkge/model.py:142-173, :402-408, :482-510):
//   M_b = reshape(W rho_b, (d, d)),  W = relation_projection.0.weight (d^2, r),  T[i][j][k] = W[i d + j][k]
//   sp rows: q_b[j] = sum_i e_b[i] M_b[i][j]        po rows: q_b[i] = sum_j M_b[i][j] e_b[j]
// and everything behind q (candidate sweep, loss, dCand, dQ) is the tile kernels' on the folded query block.  Here: the fold
// in front of them and the backward behind them, on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32).  M (B, d^2) and its gradient
// are never written to memory: a 64 x 64 tile of one slice of M lives in the accumulators of a workgroup, is scaled by the
// rows' entity element and added to the output tile -- the reference's own nesting of the sums (Linear, then bmm), so the
// rounding error is that of a length-r sum followed by a length-d sum, not of one length-(d r) sum.
//
//   t3_nested_kernel    C[b][n] = sum_o s_b[o] * (sum_kk A_b[kk] * B_o[kk][n])      rows b in 64-row tiles of ONE direction
//       fold            A = rho, s = e,  B_o[k][n] = W[idx(o, n)][k]   (sp: idx = o d + n, po: idx = n d + o)
//       d_ent           the fold of the OTHER direction with dq in place of e   (de = M dq resp. M^T dq)
//       d_rel           A = v, s = u, B_o[j][k] = W[o d + j][k]   with dM_b = u_b (x) v_b  (sp: u = e, v = dq; po: u = dq, v = e)
//     the outer index o is split over blockIdx.z (few output tiles, a long contraction); every split writes its own slab and
//     t3_reduce_kernel adds the slabs in split order.
//   t3_dw_kernel        dW[(i, j)][k] = sum_b u_b[i] v_b[j] rho_b[k]: the operand u (x) v is formed while it is staged.
// No float atomics anywhere: two runs on the same inputs are bit-identical.  Sizes off the 64 / 16 tile are zero-padded while
// the tiles are staged; nothing outside [B) x [d) x [r) is read or written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "okge_device.h"
#include "okge_kernels.h"

namespace okge {

namespace {

constexpr int TM = 64, TN = 64, TK = 16;
constexpr int LDR = TK + 4;            // [64][16] tiles (rows along the contraction): 4 * odd, the 16 x 4 operand read hits 64 banks
constexpr int LDC = 80;                // [16][64] tiles: rows 16 banks apart, 4 rows x 16 columns hit 64 banks

struct T3Nested {
    const float *W;
    const float *A[2];                 // [direction: 0 = po rows, 1 = sp rows] base of row 0 of the batch
    const float *S[2];
    int64_t      ldA[2], ldS[2];
    int32_t      so[2], sn[2];         // BNK: row of W for (o, n) = o * so + n * sn
    float       *slab;                 // [splits][B][Nn]
    int32_t      n_po, B, d, r, Kin, Nn, outer, o_per_split, tiles_po;
};

template <bool BNK>
__global__ __launch_bounds__(256) void t3_nested_kernel(const T3Nested a)
{
    __shared__ float As[TM * LDR];
    __shared__ float Bs[BNK ? TN * LDR : TK * LDC];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1;
    const int dir = (int)blockIdx.x < a.tiles_po ? 0 : 1;
    const int row0 = dir == 0 ? blockIdx.x * TM : a.n_po + ((int)blockIdx.x - a.tiles_po) * TM;
    const int row_end = dir == 0 ? a.n_po : a.B;
    const int n0 = blockIdx.y * TN;
    const int o_lo = blockIdx.z * a.o_per_split, o_hi = min(a.outer, o_lo + a.o_per_split);
    const float *__restrict__ A = a.A[dir], *__restrict__ S = a.S[dir], *__restrict__ W = a.W;
    const int64_t ldA = a.ldA[dir], ldS = a.ldS[dir];
    const int so = a.so[dir], sn = a.sn[dir];
    v4f acc[2][2], inner[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = inner[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
    float ra[4], rb[4];
    auto load = [&](int o, int k0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = row0 + (tid >> 4) + 16 * j, kk = k0 + (tid & 15);
            ra[j] = (m < row_end && kk < a.Kin) ? A[(size_t)m * ldA + kk] : 0.f;
            if (BNK) {                                   // W[idx(o, n)][kk]: 16 consecutive floats of 4 rows per wave-instruction
                const int n = n0 + (tid >> 4) + 16 * j;
                rb[j] = (n < a.Nn && kk < a.Kin) ? W[((size_t)o * so + (size_t)n * sn) * a.r + kk] : 0.f;
            } else {                                     // W[o d + kk][n]: rows of 64 consecutive n
                const int k2 = k0 + (tid >> 6) + 4 * j, n = n0 + (tid & 63);
                rb[j] = (k2 < a.Kin && n < a.Nn) ? W[((size_t)o * a.d + k2) * a.r + n] : 0.f;
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            As[((tid >> 4) + 16 * j) * LDR + (tid & 15)] = ra[j];
            if (BNK) Bs[((tid >> 4) + 16 * j) * LDR + (tid & 15)] = rb[j];
            else Bs[((tid >> 6) + 4 * j) * LDC + (tid & 63)] = rb[j];
        }
    };
    if (o_lo < o_hi) load(o_lo, 0);
    for (int o = o_lo; o < o_hi; ++o) {
        // the rows' scale for this slice: result register rr of block i belongs to row 32 wm + 16 i + 4 (lane >> 4) + rr
        float sv[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int m = row0 + 32 * wm + 16 * i + 4 * (lane >> 4) + rr;
                sv[i][rr] = m < row_end ? S[(size_t)m * ldS + o] : 0.f;
            }
        for (int k0 = 0; k0 < a.Kin; k0 += TK) {
            __syncthreads();                             // the previous chunk has been multiplied
            stage();
            __syncthreads();
            if (k0 + TK < a.Kin) load(o, k0 + TK);
            else if (o + 1 < o_hi) load(o + 1, 0);
#pragma unroll
            for (int k4 = 0; k4 < TK; k4 += 4) {
                float av[2], bv[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int kk = k4 + (lane >> 4);
                    av[i] = As[(32 * wm + 16 * i + (lane & 15)) * LDR + kk];
                    bv[i] = BNK ? Bs[(32 * wn + 16 * i + (lane & 15)) * LDR + kk] : Bs[kk * LDC + 32 * wn + 16 * i + (lane & 15)];
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) inner[i][j] = mfma16(av[i], bv[j], inner[i][j]);
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) acc[i][j][rr] = fmaf(sv[i][rr], inner[i][j][rr], acc[i][j][rr]);
                inner[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
            }
    }
    float *Cz = a.slab + (size_t)blockIdx.z * a.B * a.Nn;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int m = row0 + 32 * wm + 16 * i + 4 * (lane >> 4) + rr, n = n0 + 32 * wn + 16 * j + (lane & 15);
                if (m < row_end && n < a.Nn) Cz[(size_t)m * a.Nn + n] = acc[i][j][rr];
            }
}

// out[rows_out][ld_out]: (b < B, n < Nn) = sum of the slabs in split order, everything else (a query block's padding) zero
__global__ __launch_bounds__(256) void t3_reduce_kernel(const float *__restrict__ slab, int splits, int B, int Nn, float *__restrict__ out,
                                                        int rows_out, int64_t ld_out, int cols_out)
{
    const int64_t total = (int64_t)rows_out * cols_out, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int b = (int)(t / cols_out), n = (int)(t % cols_out);
        float v = 0.f;
        if (b < B && n < Nn)
            for (int s = 0; s < splits; ++s) v += slab[((size_t)s * B + b) * Nn + n];
        out[(size_t)b * ld_out + n] = v;
    }
}

// dW[m = i d + j][k] (+)= sum_b u_b[i] v_b[j] rho_b[k]   (po rows: u = dq, v = e; sp rows: u = e, v = dq)
__global__ __launch_bounds__(256) void t3_dw_kernel(const float *__restrict__ ent, int64_t ld_e, const float *__restrict__ dq, int64_t ld_q,
                                                    const float *__restrict__ rho, int64_t ld_r, int n_po, int B, int d, int r, int fresh,
                                                    float *__restrict__ dW)
{
    __shared__ float As[TK * LDC];
    __shared__ float Bs[TK * LDC];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1;
    const int M = d * d;
    const int m0 = blockIdx.x * TM, n0 = blockIdx.y * TN;
    const int mt = m0 + (tid & 63), nt = n0 + (tid & 63);
    const int it = mt < M ? mt / d : 0, jt = mt < M ? mt % d : 0;
    // two-level sum over the batch: 64 rows at a time in `part`, the parts added up in `acc` (the error of a length-B fp32 sum
    // grows with sqrt(B); a blocked sum keeps it at that of its longest leg)
    v4f acc[2][2], part[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = part[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
    float ra[4], rb[4];
    auto load = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = k0 + (tid >> 6) + 4 * j;
            ra[j] = rb[j] = 0.f;
            if (b < B) {
                const float *e = ent + (size_t)b * ld_e, *g = dq + (size_t)b * ld_q;
                if (mt < M) ra[j] = b < n_po ? __fmul_rn(g[it], e[jt]) : __fmul_rn(e[it], g[jt]);
                if (nt < r) rb[j] = rho[(size_t)b * ld_r + nt];
            }
        }
    };
    load(0);
    for (int k0 = 0; k0 < B; k0 += TK) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            As[((tid >> 6) + 4 * j) * LDC + (tid & 63)] = ra[j];
            Bs[((tid >> 6) + 4 * j) * LDC + (tid & 63)] = rb[j];
        }
        __syncthreads();
        if (k0 + TK < B) load(k0 + TK);
#pragma unroll
        for (int k4 = 0; k4 < TK; k4 += 4) {
            float av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int kk = k4 + (lane >> 4);
                av[i] = As[kk * LDC + 32 * wm + 16 * i + (lane & 15)];
                bv[i] = Bs[kk * LDC + 32 * wn + 16 * i + (lane & 15)];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) part[i][j] = mfma16(av[i], bv[j], part[i][j]);
        }
        if ((k0 + TK) % 64 == 0 || k0 + TK >= B) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[i][j] += part[i][j];
                    part[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
                }
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int m = m0 + 32 * wm + 16 * i + 4 * (lane >> 4) + rr, n = n0 + 32 * wn + 16 * j + (lane & 15);
                if (m < M && n < r) {
                    float *p = dW + (size_t)m * r + n;
                    *p = fresh ? acc[i][j][rr] : *p + acc[i][j][rr];
                }
            }
}

// out[b] = x_b . y_b over d elements: one wave per row, lanes stride the row, a butterfly adds them up (fixed order)
__global__ __launch_bounds__(64) void t3_rowdot_kernel(const float *__restrict__ x, int64_t ld_x, const float *__restrict__ y, int64_t ld_y,
                                                       int d, float *__restrict__ out)
{
    const int b = blockIdx.x;
    float v = 0.f;
    for (int k = threadIdx.x; k < d; k += 64) v = fmaf(x[(size_t)b * ld_x + k], y[(size_t)b * ld_y + k], v);
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (threadIdx.x == 0) out[b] = v;
}

// Off the training path (the plugin methods on MATERIALISED relation matrices, model.py:147-173): M rows are [n][ld_m] with
// M_b[i][j] at i d + j.  One workgroup per row b, plain fp32 fma chains in index order.
//   transpose = 0: out[b][j] = sum_i x_b[i] M_b[i][j]   (x^T M, the sp prefix)      transpose = 1: out[b][i] = sum_j M_b[i][j] x_b[j]
__global__ __launch_bounds__(256) void t3_apply_kernel(const float *__restrict__ M, int64_t ld_m, const float *__restrict__ x, int64_t ld_x,
                                                       int d, int transpose, float *__restrict__ out, int64_t ld_out)
{
    const int b = blockIdx.x;
    const float *Mb = M + (size_t)b * ld_m, *xb = x + (size_t)b * ld_x;
    for (int n = threadIdx.x; n < d; n += blockDim.x) {
        float v = 0.f;
        if (transpose)
            for (int j = 0; j < d; ++j) v = fmaf(Mb[(size_t)n * d + j], xb[j], v);
        else
            for (int i = 0; i < d; ++i) v = fmaf(xb[i], Mb[(size_t)i * d + n], v);
        out[(size_t)b * ld_out + n] = v;
    }
}

// out[b][i d + j] = u_b[i] v_b[j]: the gradient of a materialised relation matrix
__global__ __launch_bounds__(256) void t3_outer_kernel(const float *__restrict__ u, int64_t ld_u, const float *__restrict__ v, int64_t ld_v, int d,
                                                       float *__restrict__ out, int64_t ld_out)
{
    const int b = blockIdx.x;
    for (int m = threadIdx.x; m < d * d; m += blockDim.x)
        out[(size_t)b * ld_out + m] = __fmul_rn(u[(size_t)b * ld_u + m / d], v[(size_t)b * ld_v + m % d]);
}

int row_tiles(int n_po, int B) { return (n_po + TM - 1) / TM + (B - n_po + TM - 1) / TM; }

void launch_nested(bool bnk, T3Nested a, int splits, hipStream_t st)
{
    a.tiles_po = (a.n_po + TM - 1) / TM;
    a.o_per_split = (a.outer + splits - 1) / splits;
    const dim3 grid(row_tiles(a.n_po, a.B), (a.Nn + TN - 1) / TN, (a.outer + a.o_per_split - 1) / a.o_per_split);
    if (bnk) hipLaunchKernelGGL(t3_nested_kernel<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(t3_nested_kernel<false>, grid, dim3(256), 0, st, a);
}

void launch_reduce(const float *slab, int splits, int B, int Nn, float *out, int rows_out, int64_t ld_out, int cols_out, hipStream_t st)
{
    const int64_t total = (int64_t)rows_out * cols_out;
    hipLaunchKernelGGL(t3_reduce_kernel, dim3((unsigned)std::min<int64_t>(2048, (total + 255) / 256)), dim3(256), 0, st, slab, splits, B, Nn,
                       out, rows_out, ld_out, cols_out);
}

}  // namespace

// splits of the outer index for an output of B x Nn: enough workgroups for two per CU, at most one split per slice and 64
int tucker3_splits(int B, int Nn, int outer, int cus)
{
    const int tiles = std::max(1, ((B + TM - 1) / TM) * ((Nn + TN - 1) / TN));
    int s = std::max(1, std::min(std::min(outer, 64), (2 * cus + tiles - 1) / tiles));
    const int per = (outer + s - 1) / s;
    return (outer + per - 1) / per;
}

size_t tucker3_workspace_bytes(int B, int d, int r, int cus)
{
    // the slabs of the largest split product: B x d (fold, d_ent) or B x r (d_rel)
    const size_t a = (size_t)tucker3_splits(B, d, d, cus) * B * d, b = (size_t)tucker3_splits(B, r, d, cus) * B * r;
    return std::max(a, b) * sizeof(float) + 256;
}

// Q[rows_out][ldq] (padding zero) from the masked prefix rows; po rows first.  x = ent_rows: the fold.  `transpose` swaps the
// contracted index of both directions (x = dq: d_ent, written [B][ld_out] without padding when rows_out == B).
hipError_t launch_tucker3_fold(const float *W, const float *x, int64_t ld_x, const float *rho, int64_t ld_r, int n_po, int B, int d, int r,
                               int transpose, float *out, int rows_out, int64_t ld_out, int cols_out, float *slab, int cus, hipStream_t st)
{
    T3Nested a = {};
    a.W = W;
    a.A[0] = a.A[1] = rho; a.ldA[0] = a.ldA[1] = ld_r;
    a.S[0] = a.S[1] = x;   a.ldS[0] = a.ldS[1] = ld_x;
    // po rows contract j (row of W for (o = j, n = i) = n d + o), sp rows contract i (o d + n)
    const int po = transpose ? 1 : 0, sp = 1 - po;
    a.so[po] = 1; a.sn[po] = d;
    a.so[sp] = d; a.sn[sp] = 1;
    a.slab = slab;
    a.n_po = n_po; a.B = B; a.d = d; a.r = r; a.Kin = r; a.Nn = d; a.outer = d;
    const int splits = tucker3_splits(B, d, d, cus);
    launch_nested(true, a, splits, st);
    const int o_per = (d + splits - 1) / splits;
    launch_reduce(slab, (d + o_per - 1) / o_per, B, d, out, rows_out, ld_out, cols_out, st);
    return hipGetLastError();
}

hipError_t launch_tucker3_backward(const float *W, const float *ent, int64_t ld_e, const float *rho, int64_t ld_r, const float *dq,
                                   int64_t ld_q, int n_po, int B, int d, int r, int fresh, float *d_ent, float *d_rel, float *dW,
                                   float *slab, int cus, hipStream_t st)
{
    if (d_ent) {
        hipError_t e = launch_tucker3_fold(W, dq, ld_q, rho, ld_r, n_po, B, d, r, 1, d_ent, B, d, d, slab, cus, st);
        if (e != hipSuccess) return e;
    }
    if (d_rel) {
        T3Nested a = {};
        a.W = W;
        a.A[0] = ent; a.ldA[0] = ld_e; a.S[0] = dq;  a.ldS[0] = ld_q;      // po: u = dq, v = e
        a.A[1] = dq;  a.ldA[1] = ld_q; a.S[1] = ent; a.ldS[1] = ld_e;      // sp: u = e,  v = dq
        a.slab = slab;
        a.n_po = n_po; a.B = B; a.d = d; a.r = r; a.Kin = d; a.Nn = r; a.outer = d;
        const int splits = tucker3_splits(B, r, d, cus);
        launch_nested(false, a, splits, st);
        const int o_per = (d + splits - 1) / splits;
        launch_reduce(slab, (d + o_per - 1) / o_per, B, r, d_rel, B, r, r, st);
    }
    if (dW)
        hipLaunchKernelGGL(t3_dw_kernel, dim3((d * d + TM - 1) / TM, (r + TN - 1) / TN), dim3(256), 0, st, ent, ld_e, dq, ld_q, rho, ld_r, n_po,
                           B, d, r, fresh, dW);
    return hipGetLastError();
}

hipError_t launch_tucker3_apply(const float *M, int64_t ld_m, const float *x, int64_t ld_x, int n, int d, int transpose, float *out,
                                int64_t ld_out, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(t3_apply_kernel, dim3(n), dim3(256), 0, st, M, ld_m, x, ld_x, d, transpose, out, ld_out);
    return hipGetLastError();
}

hipError_t launch_tucker3_outer(const float *u, int64_t ld_u, const float *v, int64_t ld_v, int n, int d, float *out, int64_t ld_out,
                                hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(t3_outer_kernel, dim3(n), dim3(256), 0, st, u, ld_u, v, ld_v, d, out, ld_out);
    return hipGetLastError();
}

// score_b = s_b^T M_b o_b = s_b . (M_b o_b): the po fold of the object rows into `q` ([n][d]), then a row dot (model.py:167-171)
hipError_t launch_tucker3_triples(const float *W, const float *subj, int64_t ld_s, const float *rho, int64_t ld_r, const float *obj,
                                  int64_t ld_o, int n, int d, int r, float *q, float *slab, float *out, int cus, hipStream_t st)
{
    hipError_t e = launch_tucker3_fold(W, obj, ld_o, rho, ld_r, n, n, d, r, 0, q, n, d, d, slab, cus, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(t3_rowdot_kernel, dim3(n), dim3(64), 0, st, subj, ld_s, q, (int64_t)d, d, out);
    return hipGetLastError();
}

}  // namespace okge
