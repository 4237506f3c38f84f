// The prefix path's small HBM-bound kernels around the fused tile kernels (gfx950).  The optimizer kernels are in okge_optim.hip,
// evaluation's rank kernels in okge_rank.hip.
//   encode_queries_kernel        gather + dropout + fold (s,r)/(r,o) into one query row; extra workgroups: tile offsets of the
//                                positives, gradient clears                                 model.py:455-510, :205-216, :269-272
//   query_planes_kernel          the bf16 planes of a query block folded elsewhere
//   fold_queries_kernel          the fold alone, from already masked entity rows (sharded path)
//   slab_reduce_kernel           dQ = sum of the dQ kernel's slabs (sharded path)
//   dc_reduce_kernel             dE[candidates] (+)= sum of the tile kernel's candidate-gradient slabs
//   dc_reduce_streamk_kernel     the same for a stream-K launch of fused_tile64k_kernel
//   prefix_backward_kernel       sum dQ slabs, chain rule to s/r/o rows, scatter-add        autograd of the fold + embedding_dense_backward
//   prefix_backward_vec_kernel   its float4 form (and the loss reduction)
//   row_segment_sum_kernel       stored gradient rows added per relation / entity, no float atomics
//   loss_reduce_kernel           deterministic sum of per-workgroup loss partials           trainer.py:106 (reduction='sum')
//   kl_count_pos_kernel, kl_row_lse_kernel, merge_lse_kernel
//                                label mass and log-sum-exp per row, from tile partials / from the shards   trainer.py:99-100
//   encode_rows_kernel           table rows by id, with dropout (okge_encode_rows)
//   score_triples_kernel         per-triple score of encoded rows                           model.py:231-238, :276
#include <algorithm>

#include "okge_kernels.h"
#include "okge_tile.h"
#include "okge_eval_device.h"
#include "okge_prefix_device.h"
#include "okge_tile_grad_split.h"

namespace okge {

// One folded query row (and / or its masked entity row): gather + dropout + fold.  All threads of the workgroup take part.
__device__ __forceinline__ void encode_query_row(const float *__restrict__ E, const float *__restrict__ R, int d, int scorer,
                                                 const PrefixDev &p, int b, float *__restrict__ q, float *__restrict__ er,
                                                 int ldq)
{
    const int B = p.n_po + p.n_sp;
    RowSrc rs;
    rs.owned = false;
    if (b < B) rs = row_source(p, b);
    if (!rs.owned) {       // padding row, or a prefix whose entity lives on another rank: contributes zero
        for (int k = threadIdx.x; k < ldq; k += blockDim.x) {
            if (q) q[k] = 0.f;
            if (er) er[k] = 0.f;
        }
        return;
    }
    const DropDev &de = rs.sp ? p.drop_sp_ent : p.drop_po_ent;
    const DropDev &dr = rs.sp ? p.drop_sp_rel : p.drop_po_rel;
    const float *e = E + rs.ent * d, *r = R + rs.rel * d;
    if (sc_is_bias(scorer)) {
        // data-bias scorers (model.py:281-350): the query is a copy of the one masked row, with that slot's own dropout
        // stream; the other slot's row is not read (the entity row only where the caller wants the masked entity rows)
        const bool use_e = scorer == SC_BIAS_ENTITY;
        for (int k = threadIdx.x; k < d; k += blockDim.x) {
            const float ev = (use_e || er) ? e[k] * drop_mult1(de, rs.pos, k, d) : 0.f;
            if (q) q[k] = use_e ? ev : r[k] * drop_mult1(dr, rs.pos, k, d);
            if (er) er[k] = ev;
        }
    } else if (scorer == SC_DISTMULT) {
        for (int k = threadIdx.x; k < d; k += blockDim.x) {
            const float ev = e[k] * drop_mult1(de, rs.pos, k, d);
            if (q) q[k] = __fmul_rn(ev, __fmul_rn(r[k], drop_mult1(dr, rs.pos, k, d)));
            if (er) er[k] = ev;
        }
    } else {
        const int h = d >> 1;
        if ((h & 3) == 0 && (de.enabled || dr.enabled)) {
            // The four threads of an aligned column quad need the same four keep octets -- columns k and h + k of the
            // entity and of the relation mask (h % 4 == 0: a quad never straddles an octet) -- so each computes ONE of
            // them (a Philox call) and they trade by shuffles, instead of four Philox calls per thread.
            const int role = threadIdx.x & 3, lane0 = (threadIdx.x & 63) & ~3;
            for (int k = threadIdx.x; k < h; k += blockDim.x) {
                const float ve1 = e[k], ve2 = e[h + k], vr1 = r[k], vr2 = r[h + k];     // requested before the mask arithmetic
                const DropDev &dd = (role & 2) ? dr : de;
                const int kc = (role & 1) ? h + k : k;
                const uint32_t mine = dd.enabled ? drop_keep8(dd, rs.pos, kc >> 3, d) : 0xFFu;
                const uint32_t b_e1 = __shfl(mine, lane0), b_e2 = __shfl(mine, lane0 + 1);
                const uint32_t b_r1 = __shfl(mine, lane0 + 2), b_r2 = __shfl(mine, lane0 + 3);
                auto mult = [](const DropDev &x, uint32_t bits, int col) { return !x.enabled ? 1.f : (bits >> (col & 7) & 1u) ? x.scale : 0.f; };
                const float e1 = ve1 * mult(de, b_e1, k), e2 = ve2 * mult(de, b_e2, h + k);
                const float r1 = vr1 * mult(dr, b_r1, k), r2 = vr2 * mult(dr, b_r2, h + k);
                if (q) fold_complex(rs.sp, e1, e2, r1, r2, q[k], q[h + k]);
                if (er) { er[k] = e1; er[h + k] = e2; }
            }
        } else {
            for (int k = threadIdx.x; k < h; k += blockDim.x) {
                const float e1 = e[k] * drop_mult1(de, rs.pos, k, d), e2 = e[h + k] * drop_mult1(de, rs.pos, h + k, d);
                const float r1 = r[k] * drop_mult1(dr, rs.pos, k, d), r2 = r[h + k] * drop_mult1(dr, rs.pos, h + k, d);
                if (q) fold_complex(rs.sp, e1, e2, r1, r2, q[k], q[h + k]);
                if (er) { er[k] = e1; er[h + k] = e2; }
            }
        }
    }
    for (int k = d + threadIdx.x; k < ldq; k += blockDim.x) {
        if (q) q[k] = 0.f;
        if (er) er[k] = 0.f;
    }
}

__global__ __launch_bounds__(128) void encode_queries_kernel(const float *__restrict__ E, const float *__restrict__ R,
                                                             int d, int scorer, const PrefixDev p,
                                                             float *__restrict__ Q, int ldq, int Bpad,
                                                             float *__restrict__ ent_rows,
                                                             const int32_t *__restrict__ pos_col, int nnz,
                                                             int32_t *__restrict__ tile_ptr, int tiles, int tile_w,
                                                             int cand_col0, int tp_wgs, const ClearSpec clr,
                                                             __bf16 *__restrict__ q_planes, int KB)
{
    if ((int)blockIdx.x >= Bpad + tp_wgs) {
        // more extra workgroups (OKGE_TRAIN_CLEAR_GRADS): the gradient regions the step accumulates into without storing
        // them first -- all of dR, the rows of dE outside the candidate range -- are cleared here, one float4 per thread, in
        // the launch that precedes every kernel that adds to them (instead of two fill launches by the caller)
        int64_t i = 4 * (((int64_t)blockIdx.x - Bpad - tp_wgs) * 128 + threadIdx.x);
#pragma unroll
        for (int r = 0; r < CLEAR_REGIONS; ++r) {
            float *base = clr.p[r];
            const int64_t n = clr.n[r], n4 = (n + 3) / 4 * 4;
            if (i < n4) {
                if (i + 4 <= n && (reinterpret_cast<uintptr_t>(base + i) & 15) == 0) *reinterpret_cast<float4 *>(base + i) = make_float4(0.f, 0.f, 0.f, 0.f);
                else for (int64_t j = i; j < n && j < i + 4; ++j) base[j] = 0.f;
                return;
            }
            i -= n4;
        }
        return;
    }
    if ((int)blockIdx.x >= Bpad) {
        // extra workgroups: offsets of each candidate tile's positives in the column-sorted coordinate list
        const int t = ((int)blockIdx.x - Bpad) * 128 + threadIdx.x;
        if (t <= tiles) tile_ptr[t] = lower_bound_i32(pos_col, nnz, cand_col0 + t * tile_w);
        return;
    }
    const int b = blockIdx.x;
    encode_query_row(E, R, d, scorer, p, b, Q ? Q + (size_t)b * ldq : nullptr,      // Q == nullptr: only the masked
                     ent_rows ? ent_rows + (size_t)b * ldq : nullptr, ldq);         // entity rows are wanted
    if (Q && q_planes) {
        // the row again as three bf16 planes for the tile kernel's gradient product, from the fp32 row this workgroup just stored.
        // Other threads of the workgroup stored the elements a thread reads back here: the barrier (with its workgroup-scope fence)
        // is what makes that read legal -- it must stay between the stores above and write_query_row_planes
        __syncthreads();
        write_query_row_planes(Q + (size_t)b * ldq, d, KB, b, q_planes);
    }
}

// the query planes of a block that was folded elsewhere (okge_train_tiles)
__global__ __launch_bounds__(128) void query_planes_kernel(const float *__restrict__ Q, int ldq, int B, int d, int KB, __bf16 *__restrict__ q_planes)
{
    const int b = blockIdx.x;
    write_query_row_planes(b < B ? Q + (size_t)b * ldq : nullptr, d, KB, b, q_planes);
}

// Q[b] = fold(masked entity row b, dropout(R[rel_b])) from ALREADY MASKED entity rows (sharded path: the rows arrive
// through the all-reduce; the replicated relation table and the counter-based masks let every rank fold them itself,
// so only B x d floats cross the links instead of 2 x B x d).  Same arithmetic as encode_queries_kernel: bit-identical.
__global__ __launch_bounds__(128) void fold_queries_kernel(const float *__restrict__ R, int d, int scorer, const PrefixDev p,
                                                           const float *__restrict__ ent_rows, float *__restrict__ Q, int ldq)
{
    const int b = blockIdx.x, B = p.n_po + p.n_sp;
    float *q = Q + (size_t)b * ldq;
    if (b >= B) {
        for (int k = threadIdx.x; k < ldq; k += blockDim.x) q[k] = 0.f;
        return;
    }
    const RowSrc rs = row_source(p, b);
    const DropDev &dr = rs.sp ? p.drop_sp_rel : p.drop_po_rel;
    const float *e = ent_rows + (size_t)b * ldq, *r = R + rs.rel * d;
    if (scorer == SC_DISTMULT) {
        for (int k = threadIdx.x; k < d; k += blockDim.x) q[k] = __fmul_rn(e[k], __fmul_rn(r[k], drop_mult1(dr, rs.pos, k, d)));
    } else {
        const int h = d >> 1;
        for (int k = threadIdx.x; k < h; k += blockDim.x) {
            const float e1 = e[k], e2 = e[h + k];
            const float r1 = r[k] * drop_mult1(dr, rs.pos, k, d), r2 = r[h + k] * drop_mult1(dr, rs.pos, h + k, d);
            fold_complex(rs.sp, e1, e2, r1, r2, q[k], q[h + k]);
        }
    }
    for (int k = d + threadIdx.x; k < ldq; k += blockDim.x) q[k] = 0.f;
}

// dQ[b][k] = sum over candidate ranges of the dQ kernel's slabs (sharded path: reduced before the all-reduce)
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float *__restrict__ slab, int nsplit, int64_t n4,
                                                          float *__restrict__ out, const double *__restrict__ loss_partials,
                                                          int n_partials, double *__restrict__ loss_out)
{
    if (blockIdx.x == gridDim.x - 1) {                      // one extra workgroup: the deterministic loss reduction
        if (loss_partials) loss_reduce_block(loss_partials, n_partials, loss_out);
        return;
    }
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int sidx = 0; sidx < nsplit; ++sidx) {
        const float4 v = reinterpret_cast<const float4 *>(slab)[(size_t)sidx * n4 + i];
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    reinterpret_cast<float4 *>(out)[i] = acc;
}

// dE[candidate n] (+)= sum over the batch splits of the fused tile kernel's partial candidate-gradient slabs
// (one thread per 4 columns; rows of repeated candidate ids accumulate with atomics)
__global__ __launch_bounds__(256) void dc_reduce_kernel(const float *__restrict__ slab, int nsplit, int rows_pad, int D16,
                                                        int N, int d, const int32_t *__restrict__ cand_ids, int cand_first,
                                                        int exclusive, int grads_zero, float *__restrict__ dE,
                                                        int64_t table_rows, int *__restrict__ id_err)
{
    const int q4 = D16 >> 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)N * q4) return;
    const int n = (int)(i / q4), k = 4 * (int)(i % q4);
    if (k >= d) return;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int sidx = 0; sidx < nsplit; ++sidx) {
        const float4 v = *reinterpret_cast<const float4 *>(slab + ((size_t)sidx * rows_pad + n) * D16 + k);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    const int64_t cid = cand_table_row(cand_ids, cand_first, n, table_rows, id_err);
    float *dst = dE + cid * d + k;
    const float v[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (k + e >= d) break;
        if (!exclusive) atomicAdd(dst + e, v[e]);
        else dst[e] = grads_zero ? v[e] : dst[e] + v[e];
    }
}

// Stream-K launches of fused_tile64k_kernel (okge_train64k.hip): the (tile, chunk) units, tile-major, are cut into `P` equal
// runs; workgroup p owns units [U p / P, U (p + 1) / P), U = tiles * J.  A tile covered by ONE segment was written by that
// workgroup; otherwise every segment left its partial rows in slab 2 p (p's run starts inside the tile) or 2 p + 1 (it
// ends there).  One workgroup per tile: list the slabs (in p order: the sum is reproducible), add them, store / accumulate.
constexpr int SK_MAX_WGS = 511, SK_SLOTS = 1024;     // a tile's slab list holds at most two entries per workgroup of the launch
static_assert(SK_SLOTS >= 2 * (SK_MAX_WGS + 1), "dc_reduce_streamk_kernel: slot list too small for the largest stream-K launch");
__global__ __launch_bounds__(256) void dc_reduce_streamk_kernel(const float *__restrict__ slab, int tiles, int J, int P, int D16,
                                                                int N, int d, const int32_t *__restrict__ cand_ids,
                                                                int cand_first, int exclusive, int grads_zero,
                                                                float *__restrict__ dE, int64_t table_rows,
                                                                int *__restrict__ id_err)
{
    // grid: 8 workgroups per tile (8 candidate rows each: the launch is a 3 x 20 MB stream, it needs the whole chip)
    __shared__ int slots[SK_SLOTS];
    __shared__ int n_slots;
    const int t = blockIdx.x >> 3, r0 = 8 * (blockIdx.x & 7);
    const int64_t U = (int64_t)tiles * J, lo = (int64_t)t * J, hi = lo + J;
    if (threadIdx.x == 0) {
        int64_t p = lo * P / U;
        while (p > 0 && U * p / P > lo) --p;
        while (U * (p + 1) / P <= lo) ++p;
        int cnt = 0;
        bool whole = false;
        for (; p < P && U * p / P < hi; ++p) {
            const int64_t ub = U * p / P, ue = U * (p + 1) / P;
            const int64_t j0 = (ub > lo ? ub : lo) - lo, j1 = (ue < hi ? ue : hi) - lo;
            if (j1 <= j0) continue;
            if (j0 == 0 && j1 == J) { whole = true; break; }
            if (cnt < SK_SLOTS) slots[cnt++] = (int)(2 * p + (ub >= lo ? 0 : 1));
            else if (id_err) atomicAdd(id_err, 1);            // (unreachable: the launcher refuses P > SK_MAX_WGS; never a silent drop)
        }
        n_slots = whole ? 0 : cnt;
    }
    __syncthreads();
    const int ns = n_slots;
    if (ns == 0) return;
    const int q4 = D16 >> 2;
    for (int i = threadIdx.x; i < 8 * q4; i += 256) {
        const int r = r0 + i / q4, k = 4 * (i % q4), n = 64 * t + r;
        if (n >= N || k >= d) continue;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < ns; ++j) {
            const float4 v = *reinterpret_cast<const float4 *>(slab + ((size_t)slots[j] * 64 + r) * D16 + k);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        const int64_t cid = cand_table_row(cand_ids, cand_first, n, table_rows, k ? nullptr : id_err);
        float *dst = dE + cid * d + k;
        const float v[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (k + e >= d) break;
            if (!exclusive) atomicAdd(dst + e, v[e]);
            else dst[e] = grads_zero ? v[e] : dst[e] + v[e];
        }
    }
}

// which tables' gradient rows a prefix backward writes: both, or the one that is trained (a frozen table's buffer may be null)
constexpr int PREFIX_ENT = 1, PREFIX_REL = 2, PREFIX_BOTH = 3;

template <int PARTS = PREFIX_BOTH>
__global__ __launch_bounds__(128) void prefix_backward_kernel(const float *__restrict__ E, const float *__restrict__ R,
                                                              int d, int scorer, const PrefixDev p,
                                                              const float *__restrict__ slab, int nsplit, int Bpad,
                                                              int ldq, const float *__restrict__ ent_rows,
                                                              float *__restrict__ dE, float *__restrict__ dR, int distinct)
{
    // ent_rows (sharded path): the already masked prefix entity rows of ALL prefixes, so every rank forms the full
    // relation gradient; the entity gradient is scattered by the owner only.
    // distinct (OKGE_TRAIN_DISTINCT_PREFIX_ROWS): every prefix id occurs once -- its gradient row is stored, not accumulated
    // PARTS (OKGE_TRAIN_FREEZE_ENTITIES / _RELATIONS leave one out): the gradient rows that are formed and written
    constexpr bool want_e = (PARTS & PREFIX_ENT) != 0, want_r = (PARTS & PREFIX_REL) != 0;
    auto put = [&](float *dst, float v) {
        if (distinct) *dst = v;
        else atomicAdd(dst, v);
    };
    const int b = blockIdx.x;
    const RowSrc rs = row_source(p, b);
    if (!ent_rows && !rs.owned) return;
    const DropDev &de = rs.sp ? p.drop_sp_ent : p.drop_po_ent;
    const DropDev &dr = rs.sp ? p.drop_sp_rel : p.drop_po_rel;
    const float *e = ent_rows ? ent_rows + (size_t)b * ldq : E + rs.ent * d, *r = R + rs.rel * d;
    const bool e_masked = ent_rows != nullptr;
    float *ge = want_e ? dE + (rs.owned ? rs.ent : 0) * d : nullptr, *gr = want_r ? dR + rs.rel * d : nullptr;
    const size_t split_stride = (size_t)Bpad * ldq;
    const float *sl = slab + (size_t)b * ldq;
    if (scorer == SC_DISTMULT) {
        for (int k = threadIdx.x; k < d; k += blockDim.x) {
            float dq = 0.f;
            for (int sidx = 0; sidx < nsplit; ++sidx) dq += sl[sidx * split_stride + k];
            const float me = drop_mult1(de, rs.pos, k, d), mr = drop_mult1(dr, rs.pos, k, d);
            const float ev = e_masked ? e[k] : e[k] * me, rv = r[k] * mr;
            if (rs.owned && want_e) put(ge + k, dq * rv * me);
            if (want_r) put(gr + k, dq * ev * mr);
        }
        return;
    }
    const int h = d >> 1;
    for (int k = threadIdx.x; k < h; k += blockDim.x) {
        float q1 = 0.f, q2 = 0.f;
        for (int sidx = 0; sidx < nsplit; ++sidx) {
            q1 += sl[sidx * split_stride + k];
            q2 += sl[sidx * split_stride + h + k];
        }
        const float me1 = drop_mult1(de, rs.pos, k, d), me2 = drop_mult1(de, rs.pos, h + k, d);
        const float mr1 = drop_mult1(dr, rs.pos, k, d), mr2 = drop_mult1(dr, rs.pos, h + k, d);
        const float e1 = e_masked ? e[k] : e[k] * me1, e2 = e_masked ? e[h + k] : e[h + k] * me2;
        const float r1 = r[k] * mr1, r2 = r[h + k] * mr2;
        float de1, de2, dr1, dr2;
        if (rs.sp) {
            de1 = q1 * r1 + q2 * r2;  de2 = -q1 * r2 + q2 * r1;
            dr1 = q1 * e1 + q2 * e2;  dr2 = -q1 * e2 + q2 * e1;
        } else {
            de1 = q1 * r1 - q2 * r2;  de2 = q1 * r2 + q2 * r1;
            dr1 = q1 * e1 + q2 * e2;  dr2 = q1 * e2 - q2 * e1;
        }
        if (rs.owned && want_e) {
            put(ge + k, de1 * me1);
            put(ge + h + k, de2 * me2);
        }
        if (want_r) {
            put(gr + k, dr1 * mr1);
            put(gr + h + k, dr2 * mr2);
        }
    }
}

__global__ __launch_bounds__(256) void loss_reduce_kernel(const double *__restrict__ partials, int n,
                                                          double *__restrict__ out)
{
    loss_reduce_block(partials, n, out);
}

// One batch row per 128-thread workgroup: lane = (column group g = tid >> 2, split quarter sq = tid & 3).  The four
// lanes of a column group sum disjoint quarters of the nsplit dQ slabs (all their loads are issued at once) and
// combine with two shuffles; sq == 0 then applies the chain rule and stores its four columns, or -- on the atomic path -- hands
// one column to each lane of the group, so that a wave adds 256 contiguous bytes at a time.  Needs d % 8 == 0 (ComplEx) or
// d % 4 == 0 (DistMult).  The last workgroup (blockIdx.x == gridDim.x - 1) instead sums the loss partials.
// NB: slab loads kept in flight per lane (8 for the single-device step's 32 split-K slabs; 1 for the sharded step, whose dQ
// arrives already reduced: 89 instead of 149 registers = 5 instead of 3 waves per SIMD, which is what bounds a launch of
// 4096 one-row workgroups -- 2.7 rounds of a ~7 us dependent-load chain at 3 waves)
template <int NB, int PARTS = PREFIX_BOTH>
__global__ __launch_bounds__(128) void prefix_backward_vec_kernel(const float *__restrict__ E, const float *__restrict__ R,
                                                                  int d, int scorer, const PrefixDev p,
                                                                  const float *__restrict__ slab, int nsplit, int Bpad,
                                                                  int ldq, const float *__restrict__ ent_rows,
                                                                  float *__restrict__ dE, float *__restrict__ dR,
                                                                  const double *__restrict__ loss_partials,
                                                                  int n_partials, double *__restrict__ loss_out,
                                                                  float *__restrict__ dr_rows, float *__restrict__ de_rows,
                                                                  int distinct)
{
    // blockIdx.y: 128-column chunk of the row (rows longer than 128 floats per half: the chunks were a loop of dependent
    // round trips inside one workgroup -- 21 us at DistMult d = 512 -- and are workgroups of their own now)
    // dr_rows / de_rows ([B][ldq] each, or nullptr): the relation- / entity-gradient row of every batch row is STORED there
    // instead of being added into dR / dE with float atomics -- row_segment_sum_kernel then adds up the rows of each
    // relation / entity (okge_prefix_backward_segmented)
    if (blockIdx.x == gridDim.x - 1) {                   // the workgroup behind the batch rows: the deterministic loss reduction
        if (blockIdx.y == 0 && loss_partials) loss_reduce_block(loss_partials, n_partials, loss_out);
        return;
    }
    const int b = blockIdx.x, grp = threadIdx.x >> 2, sq = threadIdx.x & 3;
    const RowSrc rs = row_source(p, b);
    if (!ent_rows && !rs.owned) return;
    const DropDev &de = rs.sp ? p.drop_sp_ent : p.drop_po_ent;
    const DropDev &dr = rs.sp ? p.drop_sp_rel : p.drop_po_rel;
    const float *e = ent_rows ? ent_rows + (size_t)b * ldq : E + rs.ent * d, *r = R + rs.rel * d;
    const bool e_masked = ent_rows != nullptr;
    // PARTS (OKGE_TRAIN_FREEZE_ENTITIES / _RELATIONS leave one out): the gradient rows that are formed and written
    constexpr bool want_e = (PARTS & PREFIX_ENT) != 0, want_r = (PARTS & PREFIX_REL) != 0;
    float *ge = de_rows ? de_rows + (size_t)b * ldq : want_e ? dE + (rs.owned ? rs.ent : 0) * d : nullptr;
    float *gr = dr_rows ? dr_rows + (size_t)b * ldq : want_r ? dR + rs.rel * d : nullptr;
    const size_t split_stride = (size_t)Bpad * ldq;
    const float *sl = slab + (size_t)b * ldq;
    const int s_lo = (nsplit * sq) >> 2, s_hi = (nsplit * (sq + 1)) >> 2;
    // distinct (OKGE_TRAIN_DISTINCT_PREFIX_ROWS): every prefix id occurs once in the batch: the table's gradient row itself is
    // a row of its own
    // v: the lead lane's (sq == 0) four columns.  Stored by the lead lane, or added by all four lanes of the column group, one
    // column each, so that a wave adds 64 consecutive floats per instruction (quad_lead_component): every lane of the workgroup
    // calls put; act: the lane's group stands on columns of the row
    const bool store_r = dr_rows || distinct, store_e = de_rows || distinct;
    auto put = [&](bool store, float *dst, float4 v, bool act) {      // a row of its own (plain store) or an atomic add into dR / dE
        if (store) {
            if (act && sq == 0) *reinterpret_cast<float4 *>(dst) = v;
        } else {
            const float c = quad_lead_component(v, sq);
            if (act) atomicAdd(dst + sq, c);
        }
    };
    auto put2 = [&](bool store, float *dst, int h, float4 v1, float4 v2, bool act) {      // ComplEx: the same columns of both halves
        if (store) {
            if (act && sq == 0) { *reinterpret_cast<float4 *>(dst) = v1; *reinterpret_cast<float4 *>(dst + h) = v2; }
        } else {
            const float c1 = quad_lead_component(v1, sq), c2 = quad_lead_component(v2, sq);
            if (act) { atomicAdd(dst + sq, c1); atomicAdd(dst + h + sq, c2); }
        }
    };
    auto dq_sum = [&](int k, bool active) { return dq_quad_sum<NB>(sl, split_stride, s_lo, s_hi, k, active); };
    // The keep nibbles of a column group: lane sq computes ONE of the (up to four) Philox calls the group needs and the
    // chain-rule lane collects them by shuffles; the table rows are requested before the slab sums so that their round
    // trip overlaps the slabs' (ids -> {rows, slabs, masks} -> atomics instead of ids -> slabs -> masks -> rows -> atomics).
    const int lane0 = (threadIdx.x & 63) & ~3;
    auto nibble = [&](const DropDev &dd, int k, bool active) -> uint32_t {
        if (!dd.enabled) return 15u;
        return active ? (drop_keep8(dd, rs.pos, k >> 3, d) >> (k & 4)) & 15u : 0u;
    };
    auto mult4 = [&](const DropDev &dd, uint32_t nib) {
        float4 m = make_float4(1.f, 1.f, 1.f, 1.f);
        if (dd.enabled) apply_keep4(m, nib, dd.scale);
        return m;
    };
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (scorer == SC_DISTMULT) {
        for (int k0 = 128 * blockIdx.y; k0 < d; k0 += 128 * gridDim.y) {
            const int k = k0 + 4 * grp;
            const bool act = k < d, lead = act && sq == 0;
            if (!__any(act)) continue;                   // a wave past the row's last column group (a scalar branch)
            const float4 ev0 = lead ? *reinterpret_cast<const float4 *>(e + k) : zero4;
            const float4 rv0 = lead ? *reinterpret_cast<const float4 *>(r + k) : zero4;
            const uint32_t nib = nibble((sq & 1) ? dr : de, k, act && sq < 2);
            const uint32_t nib_e = __shfl(nib, lane0), nib_r = __shfl(nib, lane0 + 1);
            const float4 dq = dq_sum(act ? k : 0, act);
            // (every lane runs the chain rule -- on zero rows where it is not the lead lane -- so that no branch stands
            //  between the slab sums and the group's adds; only the lead lane's result is used)
            const float4 me = mult4(de, nib_e), mr = mult4(dr, nib_r);
            const float4 ev = e_masked ? ev0 : f4mul(ev0, me);
            const float4 rv = f4mul(rv0, mr);
            if (rs.owned && want_e) put(store_e, ge + k, f4mul(f4mul(dq, rv), me), act);
            if (want_r) put(store_r, gr + k, f4mul(f4mul(dq, ev), mr), act);
        }
        return;
    }
    const int h = d >> 1;
    for (int k0 = 128 * blockIdx.y; k0 < h; k0 += 128 * gridDim.y) {
        const int k = k0 + 4 * grp;
        const bool act = k < h, lead = act && sq == 0;
        if (!__any(act)) continue;                   // a wave past the row's last column group (a scalar branch)
        float4 e1 = zero4, e2 = zero4, r1 = zero4, r2 = zero4;
        if (lead) {
            e1 = *reinterpret_cast<const float4 *>(e + k);  e2 = *reinterpret_cast<const float4 *>(e + h + k);
            r1 = *reinterpret_cast<const float4 *>(r + k);  r2 = *reinterpret_cast<const float4 *>(r + h + k);
        }
        const uint32_t nib = nibble((sq & 2) ? dr : de, (sq & 1) ? h + k : k, act);
        const uint32_t n_e1 = __shfl(nib, lane0), n_e2 = __shfl(nib, lane0 + 1);
        const uint32_t n_r1 = __shfl(nib, lane0 + 2), n_r2 = __shfl(nib, lane0 + 3);
        const float4 q1 = dq_sum(act ? k : 0, act), q2 = dq_sum(act ? h + k : 0, act);
        const float4 me1 = mult4(de, n_e1), me2 = mult4(de, n_e2), mr1 = mult4(dr, n_r1), mr2 = mult4(dr, n_r2);
        if (!e_masked) { e1 = f4mul(e1, me1); e2 = f4mul(e2, me2); }
        r1 = f4mul(r1, mr1);
        r2 = f4mul(r2, mr2);
        float4 de1, de2, dr1, dr2;
        if (rs.sp) {
            de1 = f4fma(q1, r1, f4mul(q2, r2));           de2 = f4fma(q2, r1, f4neg(f4mul(q1, r2)));
            dr1 = f4fma(q1, e1, f4mul(q2, e2));           dr2 = f4fma(q2, e1, f4neg(f4mul(q1, e2)));
        } else {
            de1 = f4fma(q1, r1, f4neg(f4mul(q2, r2)));    de2 = f4fma(q1, r2, f4mul(q2, r1));
            dr1 = f4fma(q1, e1, f4mul(q2, e2));           dr2 = f4fma(q1, e2, f4neg(f4mul(q2, e1)));
        }
        if (rs.owned && want_e) put2(store_e, ge + k, h, f4mul(de1, me1), f4mul(de2, me2), act);
        if (want_r) put2(store_r, gr + k, h, f4mul(dr1, mr1), f4mul(dr2, mr2), act);
    }
}

// dR[relation] / dE[entity] += the gradient rows of the batch rows that name this relation / entity, in the plan's (stable)
// order: one workgroup per segment, one float4 column group per thread -- plain loads and ONE read-modify-write per table
// row, no float atomics (1.6 M of them at the 8-rank FB15k-237 shape: 4096 batch rows x 200 columns x 2 tables, 17 batch
// rows per relation) and a fixed summation order.  order[] = batch rows sorted by id, seg_ptr[] = the bounds of the runs of
// equal ids (host-built, like the exchange plan: the ids are on the host before the batch is uploaded).  Workgroups
// 0 .. n_rel_seg-1 take the relation segments, the rest the entity segments (skipped when another rank owns the entity).
struct RowSegments { const int32_t *order, *seg_ptr; int32_t n_seg; };
__global__ __launch_bounds__(128) void row_segment_sum_kernel(const float *__restrict__ dr_rows, const float *__restrict__ de_rows,
                                                              int ldq, int d, const PrefixDev p, const RowSegments rel,
                                                              const RowSegments ent, float *__restrict__ dR, float *__restrict__ dE)
{
    const bool is_rel = (int)blockIdx.x < rel.n_seg;
    const RowSegments &sg = is_rel ? rel : ent;
    const int sidx = is_rel ? blockIdx.x : blockIdx.x - rel.n_seg;
    const int B = p.n_po + p.n_sp;
    // (the plan is host-built and trusted for speed, never for safety: bounds outside [0, B] would read `order` out of range)
    const int lo = min(max(sg.seg_ptr[sidx], 0), B), hi = min(max(sg.seg_ptr[sidx + 1], 0), B);
    if (hi <= lo) return;
    const RowSrc rs = row_source(p, min(max(sg.order[lo], 0), B - 1), false);
    if (!is_rel && !rs.owned) return;
    const float *rows = is_rel ? dr_rows : de_rows;
    float *dst = is_rel ? dR + rs.rel * d : dE + rs.ent * d;
    for (int k = 4 * threadIdx.x; k < d; k += 4 * 128) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int i = lo; i < hi; ++i) {
            const int b = min(max(sg.order[i], 0), B - 1);
            const float4 v = *reinterpret_cast<const float4 *>(rows + (size_t)b * ldq + k);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        if (k + 4 <= d) {
            float4 o = *reinterpret_cast<const float4 *>(dst + k);
            o.x += acc.x; o.y += acc.y; o.z += acc.z; o.w += acc.w;
            *reinterpret_cast<float4 *>(dst + k) = o;
        } else {
            const float v[4] = {acc.x, acc.y, acc.z, acc.w};
            for (int e = 0; k + e < d; ++e) dst[k + e] += v[e];
        }
    }
}

__global__ __launch_bounds__(256) void kl_count_pos_kernel(const int32_t *__restrict__ pos_row, int nnz,
                                                           float *__restrict__ row_ysum)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < nnz && pos_row[i] >= 0) atomicAdd(row_ysum + pos_row[i], 1.0f);      // row < 0: padding (fixed-size graphs)
}

// row log-sum-exp from the per-(tile, row) (max, sum-exp) pairs of the stats pass: one wave per batch row, lanes stride
// over the tiles (a thread per row walked 2 x tiles strided loads in sequence: 98 us at 228 tiles)
__global__ __launch_bounds__(256) void kl_row_lse_kernel(const float *__restrict__ stats, int tiles, int B, int Bpad,
                                                         float2 *__restrict__ run, int first, int last,
                                                         float *__restrict__ row_lse, int row_blocks,
                                                         const int32_t *__restrict__ pos_row, int nnz,
                                                         float *__restrict__ row_ysum)
{
    if ((int)blockIdx.x >= row_blocks) {
        // extra workgroups: label mass per row (trainer.py:99-101: y is not normalised) -- row_ysum was cleared by the step's
        // first launch; this replaces a memset + a launch of its own
        const int i = ((int)blockIdx.x - row_blocks) * 256 + threadIdx.x;
        if (i < nnz && pos_row[i] >= 0) atomicAdd(row_ysum + pos_row[i], 1.0f);      // row < 0: padding (fixed-size graphs)
        return;
    }
    // candidate ranges: `run` carries the row's (max, sum of exp(x - max)) over the ranges seen so far
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    const float2 *st = reinterpret_cast<const float2 *>(stats);
    float M = -INFINITY, S = 0.f;                    // running (max, sum of exp(x - max)) of this lane's tiles
    if (!first && lane == 0) { const float2 v = run[b]; M = v.x; S = v.y; }
    for (int t = lane; t < tiles; t += 64) {
        const float2 v = st[(size_t)t * Bpad + b];
        const float m2 = fmaxf(M, v.x);
        if (m2 > -INFINITY) S = S * expf(M - m2) + v.y * expf(v.x - m2);
        M = m2;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float Mo = __shfl_xor(M, o), So = __shfl_xor(S, o);
        const float m2 = fmaxf(M, Mo);
        if (m2 > -INFINITY) S = S * expf(M - m2) + So * expf(Mo - m2);
        M = m2;
    }
    if (lane == 0) {
        if (last) row_lse[b] = M + logf(S);
        else run[b] = make_float2(M, S);
    }
}

// log-sum-exp over the shards' row log-sum-exps (sharded KL loss)
__global__ __launch_bounds__(256) void merge_lse_kernel(const float *__restrict__ parts, int world, int B, float *__restrict__ out)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float m = -INFINITY;
    for (int r = 0; r < world; ++r) m = fmaxf(m, parts[(size_t)r * B + b]);
    float sacc = 0.f;
    for (int r = 0; r < world; ++r) sacc += expf(parts[(size_t)r * B + b] - m);
    out[b] = m > -INFINITY ? m + logf(sacc) : -INFINITY;
}

__global__ __launch_bounds__(128) void encode_rows_kernel(const float *__restrict__ table, int64_t table_rows, int d,
                                                          const int32_t *__restrict__ ids, int first_id, const DropDev drop,
                                                          float *__restrict__ out, int64_t ld_out, int *__restrict__ id_err)
{
    const int i = blockIdx.x;
    const int64_t row = checked_row(ids ? (int64_t)ids[i] : (int64_t)first_id + i, table_rows, threadIdx.x == 0 ? id_err : nullptr);
    const float *src = table + row * d;
    float *dst = out + (size_t)i * ld_out;
    for (int k = threadIdx.x; k < d; k += blockDim.x) dst[k] = src[k] * drop_mult1(drop, (uint32_t)i, k, d);
}

// Per-triple score of already encoded rows, Hadamard form (model.py:231-238, :276): one wave per triple.
__global__ __launch_bounds__(256) void score_triples_kernel(const float *__restrict__ S, int64_t lds_,
                                                            const float *__restrict__ Rr, int64_t ldr,
                                                            const float *__restrict__ O, int64_t ldo, int n, int d,
                                                            int scorer, float *__restrict__ out)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const float *s = S + (size_t)i * lds_, *r = Rr + (size_t)i * ldr, *o = O + (size_t)i * ldo;
    float acc = 0.f;
    if (scorer == SC_DISTMULT) {
        for (int k = lane; k < d; k += 64) acc += s[k] * o[k] * r[k];
    } else {
        const int h = d >> 1;
        for (int k = lane; k < h; k += 64) {
            const float s1 = s[k], s2 = s[h + k], r1 = r[k], r2 = r[h + k], o1 = o[k], o2 = o[h + k];
            acc += s1 * o1 * r1 + s2 * o2 * r1 + s1 * o2 * r2 - s2 * o1 * r2;
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) out[i] = acc;
}

// ---- launchers -----------------------------------------------------------------------------------------
hipError_t launch_score_triples(const float *S, int64_t lds_, const float *Rr, int64_t ldr, const float *O, int64_t ldo,
                                int n, int d, int scorer, float *out, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(score_triples_kernel, dim3((n + 3) / 4), dim3(256), 0, st, S, lds_, Rr, ldr, O, ldo, n, d, scorer,
                       out);
    return hipGetLastError();
}

hipError_t launch_encode_queries(const float *E, const float *R, int d, int scorer, const PrefixDev &p, float *Q,
                                 int ldq, int Bpad, float *ent_rows, const int32_t *pos_col, int nnz, int32_t *tile_ptr,
                                 int tiles, int tile_w, int cand_col0, hipStream_t st, const ClearSpec *clear, v8bf *q_planes, int KB)
{
    const int extra = tile_ptr ? (tiles + 1 + 127) / 128 : 0;
    ClearSpec clr = {};
    int64_t clear_wgs = 0;
    if (clear) {
        clr = *clear;
        int64_t f4 = 0;
        for (int r = 0; r < CLEAR_REGIONS; ++r) f4 += clr.p[r] ? (clr.n[r] + 3) / 4 : 0;
        for (int r = 0; r < CLEAR_REGIONS; ++r) if (!clr.p[r]) clr.n[r] = 0;
        clear_wgs = (f4 + 127) / 128;
    }
    if (Bpad + extra + clear_wgs <= 0) return hipSuccess;
    hipLaunchKernelGGL(encode_queries_kernel, dim3((unsigned)(Bpad + extra + clear_wgs)), dim3(128), 0, st, E, R, d, scorer, p, Q,
                       ldq, Bpad, ent_rows, pos_col, nnz, tile_ptr, tiles, tile_w, cand_col0, extra, clr, reinterpret_cast<__bf16 *>(q_planes), KB);
    return hipGetLastError();
}

hipError_t launch_query_planes(const float *Q, int ldq, int B, int Bpad, int d, int KB, v8bf *q_planes, hipStream_t st)
{
    hipLaunchKernelGGL(query_planes_kernel, dim3(Bpad), dim3(128), 0, st, Q, ldq, B, d, KB, reinterpret_cast<__bf16 *>(q_planes));
    return hipGetLastError();
}

hipError_t launch_fold_queries(const float *R, int d, int scorer, const PrefixDev &p, const float *ent_rows, float *Q, int ldq,
                               int Bpad, hipStream_t st)
{
    if (Bpad <= 0) return hipSuccess;
    hipLaunchKernelGGL(fold_queries_kernel, dim3(Bpad), dim3(128), 0, st, R, d, scorer, p, ent_rows, Q, ldq);
    return hipGetLastError();
}

hipError_t launch_slab_reduce(const float *slab, int nsplit, int64_t n, float *out, const double *loss_partials,
                              int n_partials, double *loss_out, hipStream_t st)
{
    const int64_t n4 = n / 4;
    if (n4 <= 0) return hipSuccess;
    hipLaunchKernelGGL(slab_reduce_kernel, dim3((unsigned)((n4 + 255) / 256) + 1), dim3(256), 0, st, slab, nsplit, n4, out,
                       loss_partials, n_partials, loss_out);
    return hipGetLastError();
}

hipError_t launch_dc_reduce(const float *slab, int nsplit, int rows_pad, int D16, int N, int d, const int32_t *cand_ids,
                            int cand_first, int exclusive, int grads_zero, float *dE, int64_t table_rows, int *id_err,
                            hipStream_t st)
{
    const int64_t total = (int64_t)N * (D16 / 4);
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(dc_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, slab, nsplit, rows_pad, D16, N,
                       d, cand_ids, cand_first, exclusive, grads_zero, dE, table_rows, id_err);
    return hipGetLastError();
}

hipError_t launch_dc_reduce_streamk(const float *slab, int tiles, int chunks_per_tile, int workgroups, int D16, int N, int d,
                                    const int32_t *cand_ids, int cand_first, int exclusive, int grads_zero, float *dE,
                                    int64_t table_rows, int *id_err, hipStream_t st)
{
    if (tiles <= 0) return hipSuccess;
    if (workgroups > SK_MAX_WGS) return hipErrorInvalidValue;      // (slot list of a tile: at most two entries per workgroup)
    hipLaunchKernelGGL(dc_reduce_streamk_kernel, dim3(8 * tiles), dim3(256), 0, st, slab, tiles, chunks_per_tile, workgroups, D16,
                       N, d, cand_ids, cand_first, exclusive, grads_zero, dE, table_rows, id_err);
    return hipGetLastError();
}

hipError_t launch_prefix_backward(const float *E, const float *R, int d, int scorer, const PrefixDev &p,
                                  const float *slab, int nsplit, int Bpad, int ldq, const float *ent_rows, float *dE,
                                  float *dR, const double *loss_partials, int n_partials, double *loss_out,
                                  hipStream_t st, const int32_t *rel_order, const int32_t *rel_seg_ptr, int n_rel_seg,
                                  const int32_t *ent_order, const int32_t *ent_seg_ptr, int n_ent_seg, float *grad_rows,
                                  int distinct)
{
    const int B = p.n_po + p.n_sp;
    if (B <= 0) return hipSuccess;
    // a null table gradient (OKGE_TRAIN_FREEZE_ENTITIES / _RELATIONS; the entry points that train both refuse one): not formed
    const int parts = (dE ? PREFIX_ENT : 0) | (dR ? PREFIX_REL : 0);
    if (parts == 0 || (parts != PREFIX_BOTH && (grad_rows || sc_is_bias(scorer)))) return hipErrorInvalidValue;
    const bool vec = scorer == SC_COMPLEX ? (d % 8 == 0) : (d % 4 == 0);       // (ComplEx: float4 over each half)
    if (vec) {
        // grad_rows: [2][Bpad][ldq] scratch -- relation rows, then entity rows
        const bool seg_r = grad_rows && rel_order && rel_seg_ptr && n_rel_seg > 0;
        const bool seg_e = grad_rows && ent_order && ent_seg_ptr && n_ent_seg > 0;
        float *dr_rows = seg_r ? grad_rows : nullptr, *de_rows = seg_e ? grad_rows + (size_t)Bpad * ldq : nullptr;
        const int cols = scorer == SC_COMPLEX ? d / 2 : d;
        const int chunks = std::min(8, (cols + 127) / 128);
        if (sc_is_bias(scorer)) {
            if (hipError_t e = launch_bias_prefix_rows(d, scorer, p, slab, nsplit, Bpad, ldq, ent_rows, dE, dR, loss_partials,
                                                       n_partials, loss_out, dr_rows, de_rows, distinct, st); e != hipSuccess) return e;
        } else if (parts != PREFIX_BOTH) {
            // one table frozen: the instantiation that forms the other table's rows alone (the segmented form is not reached:
            // a caller with row segments trains both tables)
            auto launch = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3(B + 1, chunks), dim3(128), 0, st, E, R, d, scorer, p, slab, nsplit, Bpad, ldq, ent_rows, dE,
                                   dR, loss_partials, n_partials, loss_out, dr_rows, de_rows, distinct);
            };
            if (parts == PREFIX_REL) nsplit >= 8 ? launch(prefix_backward_vec_kernel<8, PREFIX_REL>) : launch(prefix_backward_vec_kernel<1, PREFIX_REL>);
            else nsplit >= 8 ? launch(prefix_backward_vec_kernel<8, PREFIX_ENT>) : launch(prefix_backward_vec_kernel<1, PREFIX_ENT>);
        } else if (nsplit >= 8)
            hipLaunchKernelGGL(prefix_backward_vec_kernel<8>, dim3(B + 1, chunks), dim3(128), 0, st, E, R, d, scorer, p, slab,
                               nsplit, Bpad, ldq, ent_rows, dE, dR, loss_partials, n_partials, loss_out, dr_rows, de_rows, distinct);
        else
            hipLaunchKernelGGL(prefix_backward_vec_kernel<1>, dim3(B + 1, chunks), dim3(128), 0, st, E, R, d, scorer, p, slab,
                               nsplit, Bpad, ldq, ent_rows, dE, dR, loss_partials, n_partials, loss_out, dr_rows, de_rows, distinct);
        if (seg_r || seg_e) {
            const RowSegments rel{rel_order, rel_seg_ptr, seg_r ? n_rel_seg : 0}, ent{ent_order, ent_seg_ptr, seg_e ? n_ent_seg : 0};
            hipLaunchKernelGGL(row_segment_sum_kernel, dim3(rel.n_seg + ent.n_seg), dim3(128), 0, st, dr_rows, de_rows, ldq, d, p,
                               rel, ent, dR, dE);
        }
    } else {
        if (sc_is_bias(scorer)) {
            if (hipError_t e = launch_bias_prefix_rows(d, scorer, p, slab, nsplit, Bpad, ldq, ent_rows, dE, dR, nullptr, 0, nullptr,
                                                       nullptr, nullptr, distinct, st); e != hipSuccess) return e;
        } else if (parts == PREFIX_REL)
            hipLaunchKernelGGL(prefix_backward_kernel<PREFIX_REL>, dim3(B), dim3(128), 0, st, E, R, d, scorer, p, slab, nsplit, Bpad, ldq,
                               ent_rows, dE, dR, distinct);
        else if (parts == PREFIX_ENT)
            hipLaunchKernelGGL(prefix_backward_kernel<PREFIX_ENT>, dim3(B), dim3(128), 0, st, E, R, d, scorer, p, slab, nsplit, Bpad, ldq,
                               ent_rows, dE, dR, distinct);
        else
            hipLaunchKernelGGL(prefix_backward_kernel<PREFIX_BOTH>, dim3(B), dim3(128), 0, st, E, R, d, scorer, p, slab, nsplit, Bpad, ldq,
                               ent_rows, dE, dR, distinct);
        if (loss_partials)
            hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(256), 0, st, loss_partials, n_partials, loss_out);
    }
    return hipGetLastError();
}

hipError_t launch_loss_reduce(const double *partials, int n, double *loss_out, hipStream_t st)
{
    hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(256), 0, st, partials, n, loss_out);
    return hipGetLastError();
}

hipError_t launch_kl_count_pos(const int32_t *pos_row, int nnz, int Bpad, float *row_ysum, hipStream_t st)
{
    (void)Bpad;                                        // (row_ysum was cleared by the caller's encode launch: see train_core)
    if (nnz > 0) hipLaunchKernelGGL(kl_count_pos_kernel, dim3((nnz + 255) / 256), dim3(256), 0, st, pos_row, nnz, row_ysum);
    return hipGetLastError();
}

hipError_t launch_kl_row_lse(const float *stats, int tiles, int B, int Bpad, float *run, int first, int last, float *row_lse,
                             hipStream_t st, const int32_t *pos_row, int nnz, float *row_ysum)
{
    if (tiles <= 0 || B <= 0) return hipSuccess;
    const int row_blocks = (B + 3) / 4, count_blocks = (row_ysum && nnz > 0) ? (nnz + 255) / 256 : 0;
    hipLaunchKernelGGL(kl_row_lse_kernel, dim3(row_blocks + count_blocks), dim3(256), 0, st, stats, tiles, B, Bpad,
                       reinterpret_cast<float2 *>(run), first, last, row_lse, row_blocks, pos_row, nnz, row_ysum);
    return hipGetLastError();
}

hipError_t launch_merge_lse(const float *parts, int world, int B, float *out, hipStream_t st)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(merge_lse_kernel, dim3((B + 255) / 256), dim3(256), 0, st, parts, world, B, out);
    return hipGetLastError();
}

hipError_t launch_encode_rows(const float *table, int64_t table_rows, int d, const int32_t *ids, int first_id, int n,
                              const DropDev &drop, float *out, int64_t ld_out, int *id_err, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(encode_rows_kernel, dim3(n), dim3(128), 0, st, table, table_rows, d, ids, first_id, drop, out, ld_out, id_err);
    return hipGetLastError();
}

}  // namespace okge
