// Device code shared by the tile kernels: fused_tile64_kernel (okge_train64.hip), fused_tile64k_kernel (okge_train64k.hip)
// and fused_tile_kernel (okge_train.hip).  ONE definition of the arithmetic the golden fixtures pin -- which positives
// count as labels, the BCE / KL loss element, how a candidate position becomes a checked table row, how a tile's gradient
// rows are masked and leave for dE or a slab -- so that a fix cannot land in one kernel and miss the other.  Template
// parameters are what differs between the callers; nothing here branches on which kernel it runs in.
#pragma once
#include "okge_device.h"
#include "okge_kernels.h"

namespace okge {

// the training tile kernels: 64 candidates per tile, one 8-wave workgroup
constexpr int TILE_N = 64, TILE_THREADS = 512;

template <int KB> struct TileCfg {
    static constexpr int LDK = lds_ld(16 * KB);
    static constexpr int NO = 2 * KB;                         // 8-column octets per row
    static constexpr int KEEP_LD = NO < 32 ? 32 : NO;         // keep-flag bytes per row (LDS and global)
};

// Candidate position n of a launch -> row of the entity table: the id list if there is one, else the range that starts
// at cand_first; checked against the table (checked_row: row 0 and a count in *err for an id outside it).
__device__ __forceinline__ int64_t cand_table_row(const int32_t *cand_ids, int cand_first, int n, int64_t table_rows, int *err)
{
    return checked_row(cand_ids ? (int64_t)cand_ids[n] : (int64_t)cand_first + n, table_rows, err);
}

// ---- labels -------------------------------------------------------------------------------------------------------------
// The tile's positives [pos_lo, pos_hi) of a.pos_row / a.pos_col, the first POS_CACHE of them cached in LDS as
// (row << 6 | column of the tile).
__device__ __forceinline__ void cache_tile_positives(const FusedArgs &a, uint32_t *posc, int pos_lo, int pos_cached, int n0, int tid)
{
    for (int i = tid; i < pos_cached; i += TILE_THREADS)
        posc[i] = ((uint32_t)a.pos_row[pos_lo + i] << 6) | (uint32_t)(a.pos_col[pos_lo + i] - a.cand_col0 - n0);
}

// Label bits of the chunk of ROWS batch rows that starts at row bb (bit = candidate column of the tile, word = candidate
// half x batch row) from the tile's positives: the cached ones, then whatever did not fit the cache from global memory.
// ROWS: the chunk height of the caller (64 / 32); CACHE: how many positives the caller cached.
template <int ROWS, int CACHE = POS_CACHE>
__device__ __forceinline__ void set_label_bits(const FusedArgs &a, const uint32_t *posc, int pos_lo, int pos_hi, int pos_cached,
                                               int n0, int bb, uint32_t *yb, int tid)
{
    for (int i = tid; i < pos_cached; i += TILE_THREADS) {
        const uint32_t v = posc[i];
        const int row = (int)(v >> 6) - bb;
        if (row >= 0 && row < ROWS) atomicOr(&yb[ROWS * ((v >> 5) & 1u) + row], 1u << (v & 31u));
    }
    for (int q = pos_lo + CACHE + tid; q < pos_hi; q += TILE_THREADS) {      // overflow: rare
        const int row = a.pos_row[q] - bb;
        const int col = a.pos_col[q] - a.cand_col0 - n0;
        if (row >= 0 && row < ROWS) atomicOr(&yb[ROWS * (col >> 5) + row], 1u << (col & 31));
    }
}

// ---- loss ---------------------------------------------------------------------------------------------------------------
constexpr float TILE_LOG2E = 1.4426950408889634f, TILE_LN2 = 0.6931471805599453f;

// BCE-with-logits terms of one score: ope = 1 + e^-|x| (in (1, 2]) and sig = sigmoid(x).
// v_exp_f32 / v_rcp_f32 (1 ulp each)
struct BceTerms { float ope, sig; };
__device__ __forceinline__ BceTerms bce_terms(float xv)
{
    const float e = __builtin_amdgcn_exp2f(-fabsf(xv) * TILE_LOG2E);
    const float ope = 1.f + e;
    const float rcp = __builtin_amdgcn_rcpf(ope);
    return {ope, xv >= 0.f ? rcp : e * rcp};
}

// One element of the loss epilogue: score xv of batch row `brow` against a candidate that is / is not (`pos`) one of the
// row's labels.  Returns the element's loss l -- 0 for padding (candidate past N: !nvalid, or row past b_end), looked at
// only where `edge`, the workgroup-uniform "this tile / chunk has padding", says so -- and g = dLoss/dX / normalizer.
// (l is returned, not added to the caller's sum through a reference: with the reference fused_tile64k_kernel<32, KL>
// spilled one more register.)
// (a shard's last tile also sees the positives of the next shard's first columns: masked like padding)
struct LossTerm { float l, g; };
template <int MODE>
__device__ __forceinline__ LossTerm loss_element(const FusedArgs &a, float xv, bool pos, int brow, bool edge, bool nvalid, int b_end)
{
    static_assert(MODE == MODE_TRAIN_BCE || MODE == MODE_TRAIN_KL, "a training loss");
    float gg, l;
    if (MODE == MODE_TRAIN_BCE) {
        // BCEWithLogits: max(x,0) - x*y + log1p(exp(-|x|)); d/dx = sigmoid(x) - y
        // v_log_f32 (1 ulp); 1 + e is in (1, 2]
        const float y = pos ? a.y_pos : a.y_neg;
        const BceTerms t = bce_terms(xv);
        l = fmaxf(xv, 0.f) - xv * y + __builtin_amdgcn_logf(t.ope) * TILE_LN2;
        gg = t.sig - y;
    } else {
        // KLDiv(sum)(log_softmax(x), y), y in {0,1} unnormalised (trainer.py:99-101):
        // loss = -sum_pos log_softmax; d/dx = softmax * sum_n y - y
        const int b = min(brow, a.B - 1);
        const float lsm = xv - a.row_lse[b];
        l = pos ? -lsm : 0.f;
        gg = __builtin_amdgcn_exp2f(lsm * TILE_LOG2E) * a.row_ysum[b] - (pos ? 1.f : 0.f);
    }
    if (edge) l = (nvalid && brow < b_end) ? l : 0.f;
    return {l, gg * a.inv_norm};
}

// ---- validation loss of the counting sweep (MODE_COUNT_BCE / MODE_COUNT_KL) ---------------------------------------------------
// The label-free part of a row's loss over the candidates a lane holds, as one float2 partial: BCE (sum softplus(x), sum x),
// softplus(x) = max(x, 0) + log(1 + e^-|x|) from the BCE element's own bce_terms; KL (max, sum e^(x - max)) as MODE_STATS
// forms it.  xm: the lane's scores with -inf at padding columns, which add nothing to either sum.
template <int MODE, int NV>
__device__ __forceinline__ float2 eval_loss_lane(const float (&xm)[NV])
{
    static_assert(MODE == MODE_COUNT_BCE || MODE == MODE_COUNT_KL, "a counting mode with a loss");
    if (MODE == MODE_COUNT_BCE) {
        float sp = 0.f, sx = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const bool v = xm[i] > -INFINITY;
            sp += v ? fmaxf(xm[i], 0.f) + __builtin_amdgcn_logf(bce_terms(xm[i]).ope) * TILE_LN2 : 0.f;
            sx += v ? xm[i] : 0.f;
        }
        return make_float2(sp, sx);
    }
    float m = -INFINITY, se = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) m = fmaxf(m, xm[i]);
#pragma unroll
    for (int i = 0; i < NV; ++i) se += xm[i] > -INFINITY ? __expf(xm[i] - m) : 0.f;
    return make_float2(m, se);
}

// two partials of one row -> one.  Symmetric bit for bit (a + b == b + a), so lanes that exchange partials agree.
template <int MODE>
__device__ __forceinline__ float2 eval_loss_merge(float2 p, float2 q)
{
    if (MODE == MODE_COUNT_BCE) return make_float2(p.x + q.x, p.y + q.y);
    const float m = fmaxf(p.x, q.x);
    return make_float2(m, (p.x > -INFINITY ? p.y * __expf(p.x - m) : 0.f) + (q.x > -INFINITY ? q.y * __expf(q.x - m) : 0.f));
}

// the four lanes c, c + 16, c + 32, c + 48 of a wave hold one row: all four leave with the row's partial of the wave
template <int MODE>
__device__ __forceinline__ float2 eval_loss_row4(float2 p)
{
    p = eval_loss_merge<MODE>(p, make_float2(__shfl_xor(p.x, 16), __shfl_xor(p.y, 16)));
    return eval_loss_merge<MODE>(p, make_float2(__shfl_xor(p.x, 32), __shfl_xor(p.y, 32)));
}

// Loss partial of a workgroup of 8 waves: every wave's sum (in double) into red[8], thread 0 adds them up and stores.
__device__ __forceinline__ void store_loss_partial(float lsum, double *red, double *dst, int tid)
{
    {
        const double ls = wave_sum((double)lsum);
        if ((tid & 63) == 0) red[tid >> 6] = ls;
    }
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) tot += red[i];
        *dst = tot;
    }
}

// ---- write-back ---------------------------------------------------------------------------------------------------------
// A tile's 64 gradient rows, staged in LDS as stage[64][LDK], leave: masked with the cached dropout flags keepb[64][KEEP_LDS],
// then either into slab_rows[64][16*KB] (a workgroup that holds only part of the tile's batch rows: plain 16-byte stores; a
// reduce kernel sums the slabs into dE) or, slab_rows == nullptr, into dE.  Thread (tid >> 3, tid & 7): row, octets q8 + 8 it.
template <int KB, int KEEP_LDS = TileCfg<KB>::KEEP_LD>
__device__ __forceinline__ void store_tile_gradient(const FusedArgs &a, const float *stage, const uint8_t *keepb, float *slab_rows,
                                                    int n0, int tid)
{
    using Cfg = TileCfg<KB>;
    constexpr int LDK = Cfg::LDK, NO = Cfg::NO, NOIT = (NO + 7) / 8;
    const int d = a.d, r8 = tid >> 3, q8 = tid & 7, n = n0 + r8;
    const bool vec_ok = (d & 3) == 0;
    if (a.loss_only || n >= a.N) return;
    const int64_t cid = cand_table_row(a.cand_ids, a.cand_first, n, a.n_table_rows, nullptr);
    float *drow = a.dE + cid * d;
    const bool exclusive = !slab_rows && a.cand_exclusive;    // one workgroup per entity row: plain stores
    float *srow = slab_rows ? slab_rows + (size_t)r8 * (16 * KB) : nullptr;
#pragma unroll
    for (int it = 0; it < NOIT; ++it) {
        const int o = q8 + 8 * it, k = 8 * o;
        if (o >= NO || k >= d) continue;
        v4f v[2];
        v[0] = *reinterpret_cast<const v4f *>(stage + r8 * LDK + k);
        v[1] = *reinterpret_cast<const v4f *>(stage + r8 * LDK + k + 4);
        if (a.drop_c.enabled) {
            const uint32_t bits = keepb[r8 * KEEP_LDS + o];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[0][e] *= (bits >> e & 1u) ? a.drop_c.scale : 0.f;
                v[1][e] *= (bits >> (4 + e) & 1u) ? a.drop_c.scale : 0.f;
            }
        }
        if (srow) {                                   // 16*KB columns per slab row: k + 8 <= 16*KB always
            *reinterpret_cast<v4f *>(srow + k) = v[0];
            *reinterpret_cast<v4f *>(srow + k + 4) = v[1];
            continue;
        }
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const int kk = k + 4 * hh;
            if (kk >= d) continue;
            if (exclusive && vec_ok) {
                v4f o4 = v[hh];
                if (!a.grads_zero) o4 += *reinterpret_cast<const v4f *>(drow + kk);
                *reinterpret_cast<v4f *>(drow + kk) = o4;
            } else if (exclusive) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (kk + e < d) drow[kk + e] = a.grads_zero ? v[hh][e] : drow[kk + e] + v[hh][e];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (kk + e < d) atomicAdd(drow + kk + e, v[hh][e]);
            }
        }
    }
}

}  // namespace okge
