// C ABI (include/okge.h), host side: scoring, the training step (tile kernels up to slot size 512, the wide path above, the
// row-sparse variant), the entity-sharded phases and top-k.  Argument checking, workspace carving, launch geometry (okge_plan.h);
// no kernel here.
#include <algorithm>
#include <cstdlib>

#include "okge_host.h"
#include "okge_wide.h"

using namespace okge;

// the arguments every tile launch shares, from the fields Shape and WideShape both have; Q: the folded queries.
// b_per_block: all rows (the sweeps; train_core sets its split)
template <class AnyShape>
static void fill_common(FusedArgs &a, const AnyShape &s, const okge_tables *t, const okge_candidates *c, const float *Q)
{
    std::memset(&a, 0, sizeof(a));
    a.E = c->table ? c->table : t->E;       // table the candidate rows are gathered from
    a.n_table_rows = c->table ? c->table_rows : t->n_ent;
    a.id_err = id_err_ptr();
    a.cand_ids = c->ids;
    a.cand_first = c->first_id;
    a.Q = Q;
    a.drop_c = to_dev(c->drop);
    a.d = s.d; a.N = s.N; a.B = s.B; a.Bpad = s.Bpad; a.ldq = s.ldq;
    a.b_per_block = s.Bpad;
}

void okge::fill_fused_common(FusedArgs &a, const Shape &s, const okge_tables *t, const okge_candidates *c, const float *Q)
{
    fill_common(a, s, t, c, Q);
    a.KB = s.KB; a.LDK = s.LDK;
}

namespace {

// Arguments of the tiles from `t0` on of a launch: every per-tile pointer and the candidate window move with them
FusedArgs tile_window(const FusedArgs &base, const Shape &s, int t0)
{
    FusedArgs a = base;
    a.N = base.N - t0 * NT;
    a.cand_first += t0 * NT;
    if (a.cand_ids) a.cand_ids += t0 * NT;
    a.cand_col0 += t0 * NT;
    if (a.tile_ptr) a.tile_ptr += t0;
    if (a.loss_partial) a.loss_partial += t0;
    if (a.G) a.G += (size_t)t0 * (s.Bpad / BC) * (BC * NT);
    if (a.Cm) a.Cm += (size_t)t0 * NT * s.D16;
    if (a.Cplanes) a.Cplanes += (size_t)t0 * plane_cells_per_tile(s.D16);
    if (a.X) a.X += (size_t)t0 * NT;
    if (a.stats) a.stats += (size_t)t0 * s.Bpad * 2;
    if (a.rk_slab) a.rk_slab += (size_t)t0 * a.rk_ngroups;
    if (a.tk_part) a.tk_part += (size_t)t0 * s.Bpad * a.tk_k;
    return a;
}

}  // namespace

// the score sweep (MODE_SCORE / _STATS / _COUNT / _TOPK) of p.tiles 64-candidate tiles over all B rows, as plan_sweep cut it:
// the 64 x 64 kernel up to slot size 256 (rows are independent: the tail tiles simply run as (tile, row split) workgroups);
// above, the register-tile kernel in a stream-K launch (no partial outputs to add up)
hipError_t okge::launch_sweep(const Shape &s, const SweepPlan &p, const FusedArgs &a0, hipStream_t st, int mode)
{
    if (p.sk_wgs > 0) {
        FusedArgs a = a0;
        a.sk_tiles = p.tiles;
        return launch_fused64k(mode, a, p.sk_wgs, 1, st);
    }
    if (p.tail_split < 2) return launch_fused(mode, a0, p.tiles, 1, st);
    FusedArgs am = a0;
    am.N = p.main_tiles * NT;
    if (hipError_t e = launch_fused(mode, am, p.main_tiles, 1, st); e != hipSuccess) return e;
    FusedArgs at = tile_window(a0, s, p.main_tiles);
    at.b_per_block = p.tail_b_per_block;
    return launch_fused(mode, at, p.tail_tiles, p.tail_split, st);
}

namespace {

// what a sweep needs beside its arguments: the shape and what the planner reads
struct SweepCtx {
    const Shape &s;
    int          cus;
    Knobs        knobs;
    SweepPlan    plan(int tiles) const { return plan_sweep(s, tiles, cus, knobs); }
};

// candidate range r of a call of N candidates, in tiles of tile_w: where it starts, its candidates and its tiles
struct RangeCut { int n_lo, n, tiles; };
RangeCut cut_range(const Ranges &rg, int r, int N, int tile_w)
{
    RangeCut c;
    c.n_lo = r * rg.range_n;
    c.n = std::min(rg.range_n, N - c.n_lo);
    c.tiles = (c.n + tile_w - 1) / tile_w;
    return c;
}

// Arguments of the candidates [n_lo, n_lo + n) of the call (n_lo a multiple of the tile width): local candidate 0 of the launch
// is candidate n_lo of the call.  Positives / dropout keep their global columns through cand_col0.
// loss_stride: loss partials per tile of the launch that owns base.loss_partial (the train plan's b_split; wide: the row blocks)
FusedArgs range_args(const FusedArgs &base, int n_lo, int n, int tile_w, int loss_stride)
{
    FusedArgs a = base;
    a.N = n;
    a.cand_first += n_lo;
    if (a.cand_ids) a.cand_ids += n_lo;
    a.cand_col0 += n_lo;
    if (a.tile_ptr) a.tile_ptr += n_lo / tile_w;
    if (a.loss_partial) a.loss_partial += (size_t)(n_lo / tile_w) * loss_stride;
    return a;
}

// fold the queries of a call that only sweeps (scores, top-k): no positives, no clears
int fold_for_sweep(const okge_tables *t, const okge_prefix_batch *batch, float *Q, int ldq, int Bpad, int tiles, int tile_w, hipStream_t st)
{
    const PrefixDev p = to_dev(*batch, t);
    return OKGE_TIMED("encode_queries", "encode_queries", st,
                      launch_encode_queries(t->E, t->R, t->d, t->scorer, p, Q, ldq, Bpad, nullptr, nullptr, 0, nullptr, tiles, tile_w, 0, st));
}

// per-row log-sum-exp over all candidates of the call (KL loss): one score-statistics pass per candidate range, merged
// into a running (max, sum-exp) per row; the (B, N) scores are never materialised.  stats_launch(args, tiles): the tile
// kernel's statistics mode over one range, which leaves lists_per_tile (max, sum-exp) lists per tile; l: a layout with
// off_stats and off_run.  count_*: the rows' label mass, counted by extra workgroups of the first merge launch
template <class Layout, class StatsLaunch>
int lse_ranges(const Ranges &rg, int N, int B, int Bpad, int tile_w, int lists_per_tile, const Layout &l, const FusedArgs &base, char *ws,
               float *row_lse, hipStream_t st, const char *timer, const char *what, StatsLaunch stats_launch,
               const int32_t *count_pos_row, int count_nnz, float *count_ysum)
{
    FusedArgs b = base;
    b.stats = reinterpret_cast<float *>(ws + l.off_stats);
    b.b_per_block = Bpad;
    b.tile_ptr = nullptr;
    b.loss_partial = nullptr;
    for (int r = 0; r < rg.n_ranges; ++r) {
        const RangeCut c = cut_range(rg, r, N, tile_w);
        const FusedArgs s = range_args(b, c.n_lo, c.n, tile_w, 1);
        if (int rc = OKGE_TIMED(timer, what, st, stats_launch(s, c.tiles))) return rc;
        if (int rc = OKGE_TIMED("kl_row_lse", "kl_row_lse", st,
                                launch_kl_row_lse(s.stats, lists_per_tile * c.tiles, B, Bpad, reinterpret_cast<float *>(ws + l.off_run), r == 0,
                                                  r == rg.n_ranges - 1, row_lse, st, r == 0 ? count_pos_row : nullptr, count_nnz,
                                                  r == 0 ? count_ysum : nullptr))) return rc;
    }
    return OKGE_OK;
}

// the tile kernels' pass (slot sizes up to 512): the 64x64 cut emits one (max, sum-exp) per 64-candidate tile, the register-tile
// kernel (slot sizes above 256) one per 16-candidate block
int lse_pass(const SweepCtx &cx, const Ranges &rg, const LseLayout &l, const FusedArgs &base, char *ws, float *row_lse, hipStream_t st,
             const int32_t *count_pos_row = nullptr, int count_nnz = 0, float *count_ysum = nullptr)
{
    const Shape &g = cx.s;
    return lse_ranges(rg, g.N, g.B, g.Bpad, NT, g.KB <= 16 ? 1 : 4, l, base, ws, row_lse, st, "fused_tile_stats", "fused_tile_kernel<stats>",
                      [&](const FusedArgs &s, int tiles) { return launch_sweep(g, cx.plan(tiles), s, st, MODE_STATS); },
                      count_pos_row, count_nnz, count_ysum);
}

// ---- top-k link prediction (ranges and workspace: plan_topk) ---------------------------------------------------------------
int topk_pass(const SweepCtx &cx, const TopkPlan &tp, const FusedArgs &base, char *ws, int k, const int64_t *filt_ptr,
              const int32_t *filt_col, float *out_scores, int32_t *out_cols, int32_t *out_ids, hipStream_t st)
{
    const Shape &g = cx.s;
    FusedArgs b = base;
    TopkRec *part = reinterpret_cast<TopkRec *>(ws + tp.off_part);
    b.b_per_block = g.Bpad;
    b.tk_k = k;
    b.tk_filt_ptr = filt_ptr;
    b.tk_filt_col = filt_col;
    for (int r = 0; r < tp.n_ranges; ++r) {
        const RangeCut c = cut_range(tp, r, g.N, NT);
        FusedArgs s = range_args(b, c.n_lo, c.n, NT, 1);
        const SweepPlan sp = cx.plan(c.tiles);
        if (g.KB <= 16) {
            s.tk_part = part;
            // (the name tells whether the closing round of this range was launched apart)
            if (int rc = OKGE_TIMED(sp.tail_split > 1 ? "fused_tile_topk_tail" : "fused_tile_topk", "fused_tile_kernel<topk>", st,
                                    launch_sweep(g, sp, s, st, MODE_TOPK))) return rc;
        } else {
            s.X = reinterpret_cast<float *>(ws + tp.off_X);
            s.ldx = tp.range_n;
            if (int rc = OKGE_TIMED("fused_tile_score", "fused_tile64k_kernel<score>", st, launch_sweep(g, sp, s, st, MODE_SCORE))) return rc;
            if (int rc = OKGE_TIMED("topk_cut", "topk_cut", st,
                                    launch_topk_cut(s.X, s.ldx, g.B, g.Bpad, s.N, s.cand_col0, filt_ptr, filt_col, k, part, st))) return rc;
        }
        if (int rc = timed("topk_merge", "topk_merge", st, [&] {
                TopkMergeArgs m;
                std::memset(&m, 0, sizeof(m));
                m.sc = &part->score; m.cl = &part->col; m.elem_stride = 2;
                m.L = c.tiles; m.rows_ld = g.Bpad; m.kq = k; m.B = g.B; m.k = k;
                m.first = r == 0;
                m.out_sc = out_scores; m.out_cl = out_cols;
                if (r == tp.n_ranges - 1 && out_ids) { m.out_id = out_ids; m.cand_ids = base.cand_ids; m.cand_first = base.cand_first; }
                return launch_topk_merge(m, st);
            }))
            return rc;
    }
    return OKGE_OK;
}

int check_topk_k(int32_t k)
{
    if (k < 1) return fail(OKGE_ERR_INVALID, "k must be at least 1");
    if (k > 64) return fail(OKGE_ERR_UNSUPPORTED, "top-k keeps at most 64 candidates per row");
    return OKGE_OK;
}

int check_topk(int32_t k, const okge_prefix_batch *b, const okge_candidates *c, const int64_t *filt_ptr, const int32_t *filt_col,
               int64_t n_filter, int32_t range_n, const float *out_scores, const int32_t *out_cols)
{
    if (int rc = check_topk_k(k)) return rc;
    if (c->table) return fail(OKGE_ERR_UNSUPPORTED, "top-k takes its candidates from the entity table");
    if (any_dropout(b, c)) return fail(OKGE_ERR_UNSUPPORTED, "top-k is an eval-mode call: no dropout");
    if (range_n < 0 || n_filter < 0 || (n_filter > 0 && (!filt_ptr || !filt_col))) return fail(OKGE_ERR_INVALID, "bad filter / range");
    if (!out_scores || !out_cols) return fail(OKGE_ERR_INVALID, "null output");
    return OKGE_OK;
}

// ---- what the training step shares between the tile kernels (train_core) and the wide path (wide_core) ----------------------
// OKGE_TRAIN_FREEZE_ENTITIES / _RELATIONS: the table that is not trained.  The entry point hands the cores a null dE / dR with
// the flag; with FREEZE_ENTITIES the candidate-gradient product and everything that only serves it is left out
constexpr int32_t FREEZE_FLAGS = OKGE_TRAIN_FREEZE_ENTITIES | OKGE_TRAIN_FREEZE_RELATIONS;
bool entities_frozen(int32_t flags) { return (flags & OKGE_TRAIN_FREEZE_ENTITIES) != 0 && !(flags & OKGE_TRAIN_LOSS_ONLY); }

int check_train(const okge_candidates *cand, const okge_positives *pos, int32_t loss_kind, int32_t flags, const double *loss_out,
                const float *dE, double normalizer, const float *scores, int64_t ld_scores)
{
    if (!pos || pos->nnz < 0 || (pos->nnz > 0 && (!pos->col || !pos->row))) return fail(OKGE_ERR_INVALID, "bad positives");
    if (loss_kind != OKGE_LOSS_BCE && loss_kind != OKGE_LOSS_KL) return fail(OKGE_ERR_INVALID, "unknown loss");
    if (!loss_out || (!(flags & (OKGE_TRAIN_LOSS_ONLY | OKGE_TRAIN_FREEZE_ENTITIES)) && !dE)) return fail(OKGE_ERR_INVALID, "null output");
    if (cand->table) return fail(OKGE_ERR_INVALID, "training needs candidates from the entity table");
    if (!(normalizer > 0)) return fail(OKGE_ERR_INVALID, "normalizer must be positive");
    if (scores && ld_scores < cand->n) return fail(OKGE_ERR_INVALID, "bad scores buffer");
    return OKGE_OK;
}

// The regions the encode launch clears with extra workgroups; *clear: the spec, or null when there is nothing to clear.
//   KL: the label mass per row (Bpad floats at ysum) -- counted afterwards in the statistics pass (own row log-sum-exp) or by
//   kl_count_pos (sharded: the log-sum-exp arrives from the exchange).  Not with hipMemsetAsync: inside a captured HIP graph the
//   memset node was not re-executed / ordered on replay (ROCm 7.2), the mass doubled every replay.
//   OKGE_TRAIN_CLEAR_GRADS: all of dR and the rows of dE in front of and behind the candidate range; the candidate rows are
//   stored, so the flags gain OKGE_TRAIN_GRADS_ZERO.
int train_clears(ClearSpec &clr, const ClearSpec **clear, int32_t &flags, bool kl, float *ysum, int Bpad, const okge_tables *t,
                 const okge_shard *sh, const okge_candidates *cand, float *dE, float *dR)
{
    clr = {};
    const bool clear_grads = (flags & OKGE_TRAIN_CLEAR_GRADS) != 0 && !(flags & OKGE_TRAIN_LOSS_ONLY);
    if (clear_grads) {
        if (cand->ids || sh || (!dR && !(flags & OKGE_TRAIN_FREEZE_RELATIONS)))
            return fail(OKGE_ERR_INVALID, "OKGE_TRAIN_CLEAR_GRADS needs a contiguous candidate range on an unsharded table");
        flags |= OKGE_TRAIN_GRADS_ZERO;
        const int64_t d64 = t->d, hi = (int64_t)cand->first_id + cand->n;
        // (a frozen table's buffer is null here: nothing of it is cleared)
        if (dR) { clr.p[0] = dR;            clr.n[0] = (int64_t)t->n_rel * d64; }
        if (dE) {
            clr.p[1] = dE;                  clr.n[1] = (int64_t)cand->first_id * d64;
            clr.p[2] = dE + hi * d64;       clr.n[2] = ((int64_t)t->n_ent - hi) * d64;
        }
    }
    if (kl) { clr.p[3] = ysum; clr.n[3] = Bpad; }
    *clear = (clear_grads || kl) ? &clr : nullptr;
    return OKGE_OK;
}

// label smoothing (trainer.py:103-105): y <- (y + 1/N) * (1 - eps), bce branch only; N = n_smooth, all candidates of the step
void train_targets(FusedArgs &a, int32_t loss_kind, float label_smoothing, int n_smooth)
{
    a.y_pos = 1.f; a.y_neg = 0.f;
    if (loss_kind == OKGE_LOSS_BCE && label_smoothing > 0.f) {
        const float invn = 1.0f / (float)n_smooth;
        a.y_pos = (1.0f + invn) * (1.0f - label_smoothing);
        a.y_neg = (0.0f + invn) * (1.0f - label_smoothing);
    }
}

// the train-mode arguments both cores set; tptr / G / loss_partial: their regions of the workspace
void fill_train_common(FusedArgs &a, const okge_candidates *cand, const okge_positives *pos, int32_t loss_kind, double normalizer,
                       int32_t flags, int ldg, const int32_t *tptr, float *G, double *loss_partial, float *dE)
{
    a.ldg = ldg;
    a.pos_col = pos->col; a.pos_row = pos->row; a.nnz = pos->nnz;
    a.tile_ptr = tptr;
    a.grads_zero = (flags & OKGE_TRAIN_GRADS_ZERO) ? 1 : 0;
    // an explicit id list may name an entity twice (precompute_batch_shared_inputs takes any list): its rows are then
    // accumulated with atomics unless the caller vouches for uniqueness (the collator's lists are unique)
    a.cand_exclusive = (!cand->ids || (flags & OKGE_TRAIN_UNIQUE_CANDIDATES)) ? 1 : 0;
    a.loss_only = (flags & OKGE_TRAIN_LOSS_ONLY) ? 1 : 0;
    a.G = G;
    a.dE = dE;
    a.loss_partial = loss_partial;
    a.loss_kind = loss_kind;
    a.inv_norm = (float)(1.0 / normalizer);
}

// OKGE_TRAIN_LOSS_ONLY: the step ends with the deterministic loss reduction
int loss_only_tail(const FusedArgs &a, int n_loss_partials, double *loss_out, hipStream_t st)
{
    return OKGE_TIMED("loss_reduce", "loss_reduce", st, launch_loss_reduce(a.loss_partial, n_loss_partials, loss_out, st));
}

// the step's prefix backward from the dQ slabs, + the deterministic loss reduction (one extra workgroup)
int train_prefix_backward(const okge_tables *t, const okge_shard *sh, const okge_prefix_batch *batch, const float *slab, int nsplit, int Bpad,
                          int ldq, const FusedArgs &a, int n_loss_partials, double *loss_out, float *dR, int32_t flags, hipStream_t st)
{
    ScopedTimer tm("prefix_backward", st);
    const PrefixDev p = to_dev(*batch, t, sh);
    return hip_ok(launch_prefix_backward(t->E, t->R, t->d, t->scorer, p, slab, nsplit, Bpad, ldq, nullptr, a.dE, dR, a.loss_partial,
                                         n_loss_partials, loss_out, st, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr,
                                         (flags & OKGE_TRAIN_DISTINCT_PREFIX_ROWS) ? 1 : 0),
                  "prefix_backward");
}

// ---- the wide path: slot sizes 513 .. 4096 (okge_wide.hip; shapes, plan and layouts: okge_plan.h) ---------------------------
int wide_score(const okge_tables *t, const okge_prefix_batch *batch, const okge_candidates *cand, float *scores, int64_t ld_scores,
               void *workspace, size_t workspace_bytes, void *stream)
{
    WideShape g;
    if (!make_wide_shape(batch->n_po + batch->n_sp, cand->n, t->d, g)) return fail(OKGE_ERR_INVALID, "bad shape");
    const WideScoreLayout l = wide_score_layout(g);
    if (!workspace || workspace_bytes < l.total) return fail(OKGE_ERR_WORKSPACE, "workspace too small");
    hipStream_t st = as_stream(stream);
    float *Q = reinterpret_cast<float *>(static_cast<char *>(workspace) + l.off_Q);
    if (int rc = fold_for_sweep(t, batch, Q, g.ldq, g.Bpad, g.tiles, WIDE_TN, st)) return rc;
    FusedArgs a;
    fill_common(a, g, t, cand, Q);
    a.X = scores;
    a.ldx = ld_scores;
    // (grid.y carries the tiles: sweep the candidates in launches of at most 32768 tiles)
    constexpr int MAX_TILES = 32768;
    for (int t0 = 0; t0 < g.tiles; t0 += MAX_TILES) {
        FusedArgs s = range_args(a, t0 * WIDE_TN, std::min(g.N - t0 * WIDE_TN, MAX_TILES * WIDE_TN), WIDE_TN, g.row_blocks);
        s.X = scores + (size_t)t0 * WIDE_TN;
        if (int rc = OKGE_TIMED("wide_tile_score", "wide_tile_kernel<score>", st,
                                launch_wide_tile(MODE_SCORE, s, g.row_blocks, std::min(g.tiles - t0, MAX_TILES), st))) return rc;
    }
    return OKGE_OK;
}

// okge_train_forward_backward at slot sizes 513 .. 4096.  Per call: fold the queries (+ tile offsets of the positives, + the
// clears); KL: a statistics pass over all ranges -> row log-sum-exp.  Per candidate range: the train tile launch (loss partials,
// G), dC = G^T . Q -> dE, dQ (+)= G . Cm.  Then the prefix backward with the loss reduction.  No host synchronisation, no
// allocation, no memset node: capturable.
int wide_core(const okge_tables *t, const okge_prefix_batch *batch, const okge_candidates *cand, const okge_positives *pos,
              int32_t loss_kind, float label_smoothing, double normalizer, int32_t flags, double *loss_out, float *dE, float *dR,
              float *scores, int64_t ld_scores, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = check_train(cand, pos, loss_kind, flags, loss_out, dE, normalizer, scores, ld_scores)) return rc;
    const bool loss_only = (flags & OKGE_TRAIN_LOSS_ONLY) != 0;
    const int B = batch->n_po + batch->n_sp;
    WideShape g;
    if (!make_wide_shape(B, cand->n, t->d, g)) return fail(OKGE_ERR_INVALID, "bad shape");
    const WidePlan pl = plan_wide(g, read_knobs());
    const WideTrainLayout l = wide_train_layout(g, pl);
    if (!workspace || workspace_bytes < l.total) return fail(OKGE_ERR_WORKSPACE, "workspace too small");
    if (pl.range_tiles > 65535) return fail(OKGE_ERR_UNSUPPORTED, "candidate range too long for one launch: lower OKGE_GT_MBYTES");
    char *ws = static_cast<char *>(workspace);
    const bool kl = loss_kind == OKGE_LOSS_KL;
    float *row_lse = reinterpret_cast<float *>(ws + l.off_lse), *ysum = reinterpret_cast<float *>(ws + l.off_ysum);
    ClearSpec clr;
    const ClearSpec *clear;
    if (int rc = train_clears(clr, &clear, flags, kl, ysum, g.Bpad, t, nullptr, cand, dE, dR)) return rc;
    hipStream_t st = as_stream(stream);
    float *Q = reinterpret_cast<float *>(ws + l.off_Q);
    int32_t *tptr = reinterpret_cast<int32_t *>(ws + l.off_tptr);
    // folded queries + per-tile offsets into the column-sorted positives + the clears
    if (int rc = timed("encode_queries", "encode_queries", st, [&] {
            const PrefixDev p = to_dev(*batch, t);
            return launch_encode_queries(t->E, t->R, t->d, t->scorer, p, Q, g.ldq, g.Bpad, nullptr, pos->col, pos->nnz, tptr, g.tiles,
                                         WIDE_TN, 0, st, clear);
        }))
        return rc;
    FusedArgs a;
    fill_common(a, g, t, cand, Q);
    fill_train_common(a, cand, pos, loss_kind, normalizer, flags, pl.ldg, tptr, reinterpret_cast<float *>(ws + l.off_G),
                      reinterpret_cast<double *>(ws + l.off_loss), dE);
    train_targets(a, loss_kind, label_smoothing, cand->n);
    auto range = [&](int r) { return cut_range(pl, r, g.N, WIDE_TN); };
    if (scores) {
        for (int r = 0; r < pl.n_ranges; ++r) {
            const RangeCut c = range(r);
            FusedArgs s = range_args(a, c.n_lo, c.n, WIDE_TN, g.row_blocks);
            s.tile_ptr = nullptr; s.loss_partial = nullptr;
            s.X = scores + c.n_lo; s.ldx = ld_scores;
            if (int rc = OKGE_TIMED("wide_tile_score", "wide_tile_kernel<score>", st,
                                    launch_wide_tile(MODE_SCORE, s, g.row_blocks, c.tiles, st))) return rc;
        }
    }
    if (kl) {
        // row log-sum-exp over ALL candidates first: (max, sum-exp) per (tile, row) of a range, merged in tile and range order
        if (int rc = lse_ranges(pl, g.N, g.B, g.Bpad, WIDE_TN, 1, l, a, ws, row_lse, st, "wide_tile_stats", "wide_tile_kernel<stats>",
                                [&](const FusedArgs &s, int tiles) { return launch_wide_tile(MODE_STATS, s, g.row_blocks, tiles, st); },
                                pos->row, pos->nnz, ysum))
            return rc;
        a.row_lse = row_lse;
        a.row_ysum = ysum;
    }
    const int mode = kl ? MODE_TRAIN_KL : MODE_TRAIN_BCE;
    const bool frozen_e = entities_frozen(flags);
    const bool dropping = cand->drop.p > 0.f;
    const bool slice = !cand->ids && !dropping;              // the range's masked rows ARE a slice of the table
    float *Cm = reinterpret_cast<float *>(ws + l.off_Cm), *dC = reinterpret_cast<float *>(ws + l.off_dC);
    float *dQ = reinterpret_cast<float *>(ws + l.off_dQ), *slab = reinterpret_cast<float *>(ws + l.off_slab);
    for (int r = 0; r < pl.n_ranges; ++r) {
        const RangeCut c = range(r);
        const int n_lo = c.n_lo, n_r = c.n;
        const FusedArgs ar = range_args(a, n_lo, n_r, WIDE_TN, g.row_blocks);
        if (int rc = OKGE_TIMED("wide_tile_train", "wide_tile_kernel<train>", st, launch_wide_tile(mode, ar, g.row_blocks, c.tiles, st))) return rc;
        if (loss_only) continue;
        const float *c_op = t->E + (size_t)(cand->first_id + n_lo) * t->d;
        int64_t ld_c = t->d;
        if (!slice) {
            if (int rc = OKGE_TIMED("wide_gather", "wide_gather", st,
                                    launch_wide_gather(t->E, ar.cand_ids, ar.cand_first, n_lo, n_r, t->d, g.ldq, a.drop_c, a.n_table_rows, Cm,
                                                       st))) return rc;
            c_op = Cm; ld_c = g.ldq;
        }
        // dC = G^T . Q.  A plain slice on zero gradients: the product's rows ARE the rows of dE
        // (a frozen entity table: neither the product nor the scatter of its rows)
        const bool direct = slice && a.grads_zero;
        if (!frozen_e) {
            if (int rc = OKGE_TIMED("wide_dc_gemm", "gemm_f32_kernel<dC>", st,
                                    launch_gemm_f32(true, a.G, pl.ldg, Q, g.ldq, direct ? dE + (size_t)(cand->first_id + n_lo) * t->d : dC,
                                                    direct ? (int64_t)t->d : (int64_t)g.ldq, n_r, t->d, g.B, 1, g.B, 0, st))) return rc;
            if (!direct)
                if (int rc = OKGE_TIMED("wide_dc_scatter", "wide_dc_scatter", st,
                                        launch_wide_dc_scatter(dC, g.ldq, ar.cand_ids, ar.cand_first, n_lo, n_r, t->d, a.drop_c,
                                                               a.cand_exclusive, a.grads_zero, dE, a.n_table_rows, st))) return rc;
        }
        if (int rc = OKGE_TIMED("wide_dq_gemm", "gemm_f32_kernel<dQ>", st,
                                launch_gemm_f32(false, a.G, pl.ldg, c_op, ld_c, slab, g.ldq, g.B, t->d, n_r, pl.dq_splits, pl.dq_k_per,
                                                (int64_t)g.Bpad * g.ldq, st))) return rc;
        if (int rc = OKGE_TIMED("wide_dq_reduce", "wide_dq_reduce", st,
                                launch_wide_dq_reduce(slab, pl.dq_splits, (int64_t)g.Bpad * g.ldq, g.B, t->d, g.ldq, r > 0, dQ, st))) return rc;
    }
    if (loss_only) return loss_only_tail(a, pl.n_loss_partials, loss_out, st);
    return train_prefix_backward(t, nullptr, batch, dQ, 1, g.Bpad, g.ldq, a, pl.n_loss_partials, loss_out, dR, flags, st);
}

// Shared core of the single-device step and of the sharded okge_train_tiles.
//   q_ext   : folded queries computed elsewhere (sharded path) or nullptr (encode them here from `batch`)
//   dq_out  : if set, the dQ slabs are reduced into it and the prefix backward is left to the caller
int train_core(const okge_tables *t, const okge_shard *sh, const okge_prefix_batch *batch, const float *q_ext,
               int64_t ldq_ext, int32_t B, const okge_candidates *cand, const okge_positives *pos,
               int32_t loss_kind, float label_smoothing, double normalizer, int32_t n_cand_global, int32_t flags,
               double *loss_out, float *dE, float *dR, float *dq_out, float *scores, int64_t ld_scores,
               const float *row_lse_ext, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = check_train(cand, pos, loss_kind, flags, loss_out, dE, normalizer, scores, ld_scores)) return rc;
    const bool loss_only = (flags & OKGE_TRAIN_LOSS_ONLY) != 0;
    Shape g;
    if (!make_shape(B, cand->n, t->d, g)) return fail(OKGE_ERR_INVALID, "bad shape");
    const SweepCtx cx = {g, cu_count(), read_knobs()};
    const TrainPlan pl = plan_train(g, cx.cus, cx.knobs);
    const TrainLayout l = train_layout(g, pl);
    if (!workspace || workspace_bytes < l.total) return fail(OKGE_ERR_WORKSPACE, "workspace too small");
    if (q_ext && ldq_ext != g.ldq) return fail(OKGE_ERR_INVALID, "query block leading dimension must be okge_query_ld(d)");
    char *ws = static_cast<char *>(workspace);
    const bool kl = loss_kind == OKGE_LOSS_KL;
    float *ysum = reinterpret_cast<float *>(ws + l.off_ysum);
    ClearSpec clr;
    const ClearSpec *clear;
    if (int rc = train_clears(clr, &clear, flags, kl, ysum, g.Bpad, t, sh, cand, dE, dR)) return rc;
    hipStream_t st = as_stream(stream);
    const int cand_col0 = sh ? sh->cand_col0 : 0;
    int32_t *tptr = reinterpret_cast<int32_t *>(ws + l.off_tptr);
    {
        // folded queries (unless supplied) + per-tile offsets into the column-sorted positives + the clears
        ScopedTimer tm("encode_queries", st);
        PrefixDev p;
        std::memset(&p, 0, sizeof(p));
        if (!q_ext) p = to_dev(*batch, t, sh);
        // the tile kernel's two products read Q as three bf16 planes (and nothing else): written by the launch that folds the
        // rows, or from the caller's block by a launch of its own
        v8bf *q_planes = tile_grad_split(g.KB) ? reinterpret_cast<v8bf *>(ws + l.off_Qp) : nullptr;
        if (int rc = hip_ok(launch_encode_queries(t->E, t->R, t->d, t->scorer, p, reinterpret_cast<float *>(ws + l.off_Q), g.ldq,
                                                  q_ext ? 0 : g.Bpad, nullptr, pos->col, pos->nnz, tptr, g.tiles, NT, cand_col0, st, clear,
                                                  q_planes, g.KB),
                            "encode_queries"))
            return rc;
        if (q_ext && q_planes)
            if (int rc = hip_ok(launch_query_planes(q_ext, g.ldq, B, g.Bpad, g.d, g.KB, q_planes, st), "query_planes")) return rc;
    }
    FusedArgs a;
    fill_fused_common(a, g, t, cand, q_ext ? q_ext : reinterpret_cast<const float *>(ws + l.off_Q));
    fill_train_common(a, cand, pos, loss_kind, normalizer, flags, pl.ldg, tptr, reinterpret_cast<float *>(ws + l.off_GT),
                      reinterpret_cast<double *>(ws + l.off_loss), dE);
    train_targets(a, loss_kind, label_smoothing, n_cand_global > 0 ? n_cand_global : cand->n);
    a.b_per_block = pl.b_per_block;
    a.cand_col0 = cand_col0;
    if (g.KB <= 13) a.Cplanes = reinterpret_cast<v8bf *>(ws + l.off_Cm);
    else a.Cm = reinterpret_cast<float *>(ws + l.off_Cm);
    if (tile_grad_split(g.KB)) a.Qplanes = reinterpret_cast<const v8bf *>(ws + l.off_Qp);
    a.dC_slab = pl.dc_slabs > 0 ? reinterpret_cast<float *>(ws + l.off_dcs) : nullptr;
    if (scores) {
        FusedArgs s = a;
        s.X = scores; s.ldx = ld_scores;
        s.x_vec_ok = x_vec_ok(scores, ld_scores);
        s.b_per_block = g.Bpad;
        if (int rc = OKGE_TIMED("fused_tile_score", "fused_tile_kernel<score>", st, launch_sweep(g, cx.plan(g.tiles), s, st))) return rc;
    }
    if (kl) {
        if (sh && !row_lse_ext)
            return fail(OKGE_ERR_INVALID, "sharded KL loss: pass the all-shard row log-sum-exp (okge_row_logsumexp + exchange)");
        if (!row_lse_ext) {
            // (the label mass per row, trainer.py:99-101, is counted by extra workgroups of the pass' first kl_row_lse launch;
            //  its buffer was cleared by the encode launch above)
            if (int rc = lse_pass(cx, pl, l, a, ws, reinterpret_cast<float *>(ws + l.off_lse), st, pos->row, pos->nnz, ysum)) return rc;
        } else {
            // label mass per row (trainer.py:99-101: y is not normalised)
            if (int rc = OKGE_TIMED("kl_count_pos", "kl_count_pos", st, launch_kl_count_pos(pos->row, pos->nnz, g.Bpad, ysum, st))) return rc;
        }
        a.row_lse = row_lse_ext ? row_lse_ext : reinterpret_cast<const float *>(ws + l.off_lse);
        a.row_ysum = ysum;
    }
#ifdef OKGE_STAMPS
    if (const char *sp = std::getenv("OKGE_STAMPS_PTR")) a.stamps_dbg = reinterpret_cast<unsigned long long *>(std::strtoull(sp, nullptr, 0));
#endif
    DqArgs q;
    std::memset(&q, 0, sizeof(q));
    q.G = a.G; q.Cm = a.Cm; q.Cplanes = a.Cplanes;
    q.slab = reinterpret_cast<float *>(ws + l.off_slab);
    q.d = g.d; q.KB = g.KB; q.LDK = g.LDK; q.Bpad = g.Bpad; q.ldq = g.ldq; q.ldg = pl.ldg;
    q.nsplit = pl.nsplit;
    // a frozen entity table: the instantiation without the candidate-gradient product, in the same launch geometry (the loss
    // partials and G are those of the unfrozen call), and none of the launches that add its partial rows up
    const bool frozen_e = entities_frozen(flags);
    const int mode = frozen_e ? (kl ? MODE_TRAIN_KL_NODC : MODE_TRAIN_BCE_NODC) : (kl ? MODE_TRAIN_KL : MODE_TRAIN_BCE);
    for (int r = 0; r < pl.n_ranges; ++r) {
        const RangeCut c = cut_range(pl, r, g.N, NT);
        const int tiles_r = c.tiles;
        const FusedArgs ar = range_args(a, c.n_lo, c.n, NT, pl.b_split);
        const int tail_r = (r == pl.n_ranges - 1 && pl.tail_split > 1) ? pl.tail_tiles : 0;     // tiles of this range launched apart
        FusedArgs at = ar;
        if (int rc = timed("fused_tile_train", "fused_tile_kernel<train>", st, [&] {
                if (pl.sk_wgs > 0) {                     // stream-K: a.sk_tiles tiles x sk_chunks chunks over sk_wgs workgroups
                    FusedArgs as = ar;
                    as.sk_tiles = tiles_r;
                    return launch_fused64(mode, as, pl.sk_wgs, 1, st);
                }
                if (tail_r == 0) return launch_fused64(mode, ar, tiles_r, pl.b_split, st);
                const int main_r = tiles_r - tail_r;
                if (main_r > 0) {
                    FusedArgs am = ar;
                    am.N = main_r * NT;
                    if (hipError_t e = launch_fused64(mode, am, main_r, 1, st); e != hipSuccess) return e;
                }
                at = tile_window(ar, g, main_r);
                at.b_per_block = pl.tail_b_per_block;
                return launch_fused64(mode, at, tail_r, pl.tail_split, st);
            }))
            return rc;
        if (loss_only) continue;
        if (!frozen_e) {                             // the launches that add partial candidate gradients up
            if (tail_r > 0)
                if (int rc = OKGE_TIMED("dc_reduce", "dc_reduce", st,
                                        launch_dc_reduce(a.dC_slab, pl.dc_slabs, pl.dc_slab_rows, g.D16, at.N, g.d, at.cand_ids, at.cand_first,
                                                         a.cand_exclusive, a.grads_zero, dE, a.n_table_rows, a.id_err, st))) return rc;
            if (pl.sk_wgs > 0) {
                if (int rc = OKGE_TIMED("dc_reduce", "dc_reduce_streamk", st,
                                        launch_dc_reduce_streamk(a.dC_slab, tiles_r, pl.sk_chunks, pl.sk_wgs, g.D16, ar.N, g.d, cand->ids,
                                                                 cand->first_id, a.cand_exclusive, a.grads_zero, dE, a.n_table_rows, a.id_err,
                                                                 st))) return rc;
            } else if (pl.b_split > 1) {             // (few candidate tiles: always a single range)
                if (int rc = OKGE_TIMED("dc_reduce", "dc_reduce", st,
                                        launch_dc_reduce(a.dC_slab, pl.dc_slabs, pl.dc_slab_rows, g.D16, g.N, g.d, cand->ids, cand->first_id,
                                                         a.cand_exclusive, a.grads_zero, dE, a.n_table_rows, a.id_err, st))) return rc;
            }
        }
        q.N = ar.N;
        q.accumulate = r > 0 ? 1 : 0;           // later ranges add to the slabs of the first
        if (int rc = OKGE_TIMED("dq", "dq_kernel", st, launch_dq(q, (g.Bpad / BC) * pl.nsplit, st))) return rc;
    }
    if (loss_only) return loss_only_tail(a, pl.n_loss_partials, loss_out, st);
    if (dq_out)                                 // + the deterministic loss reduction (one extra workgroup)
        return OKGE_TIMED("slab_reduce", "slab_reduce", st,
                          launch_slab_reduce(q.slab, pl.nsplit, (int64_t)g.Bpad * g.ldq, dq_out, a.loss_partial, pl.n_loss_partials, loss_out, st));
    return train_prefix_backward(t, sh, batch, q.slab, pl.nsplit, g.Bpad, g.ldq, a, pl.n_loss_partials, loss_out, dR, flags, st);
}

// ---- OKGE_TRAIN_ROW_GRADS: gradients in occurrence rows ---------------------------------------------------------------------
// The occurrence rows of the batch are gathered into two small tables behind the step's own scratch -- EV = [candidate rows |
// prefix entity rows], RV = relation rows -- and the step runs on them with positions for ids: a contiguous candidate range
// 0 .. N-1 and OKGE_TRAIN_DISTINCT_PREFIX_ROWS, the path the encoded-row ("virtual table") models take.  Every gradient row is
// then STORED once, at its position; the tile kernels are the ones every other caller runs, untouched.  Dropout counters are
// keyed by position (okge_dropout), so the masks are the dense step's.
int train_row_grads(const okge_tables *t, const okge_prefix_batch *batch, const okge_candidates *cand, const okge_positives *pos,
                    int32_t loss_kind, float label_smoothing, double normalizer, int32_t flags, double *loss_out, float *dE,
                    float *dR, float *scores, int64_t ld_scores, void *workspace, size_t workspace_bytes, void *stream)
{
    if (flags & OKGE_TRAIN_LOSS_ONLY) return fail(OKGE_ERR_INVALID, "OKGE_TRAIN_ROW_GRADS asks for gradients: not with OKGE_TRAIN_LOSS_ONLY");
    if (cand->table) return fail(OKGE_ERR_INVALID, "training needs candidates from the entity table");
    if (!dE || !dR) return fail(OKGE_ERR_INVALID, "null output");
    if (int rc = refuse_bias(t->scorer, "okge_train_forward_backward(OKGE_TRAIN_ROW_GRADS)", "the unused slot's rows have no gradient to store")) return rc;
    const int B = batch->n_po + batch->n_sp, N = cand->n;
    Shape g;
    if (!make_shape(B, N, t->d, g)) return fail(OKGE_ERR_INVALID, "bad shape");
    const size_t train_total = train_layout(g, plan_train(g, cu_count(), read_knobs())).total;
    const RowGradsLayout l = row_grads_layout(g, train_total);
    if (!workspace || workspace_bytes < l.total) return fail(OKGE_ERR_WORKSPACE, "workspace too small (okge_train_row_grads_workspace_bytes)");
    hipStream_t st = as_stream(stream);
    char *ws = static_cast<char *>(workspace);
    RowsGather a;
    std::memset(&a, 0, sizeof(a));
    a.E = t->E; a.R = t->R;
    a.EV = reinterpret_cast<float *>(ws + l.off_EV); a.RV = reinterpret_cast<float *>(ws + l.off_RV);
    a.pos_ids = reinterpret_cast<int32_t *>(ws + l.off_ids);
    a.cand_ids = cand->ids; a.cand_first = cand->first_id; a.N = N;
    a.po_obj = batch->po_obj; a.sp_subj = batch->sp_subj; a.po_rel = batch->po_rel; a.sp_rel = batch->sp_rel;
    a.n_po = batch->n_po; a.n_sp = batch->n_sp; a.d = t->d;
    a.n_ent = t->n_ent; a.n_rel = t->n_rel;
    a.id_err = id_err_ptr();
    a.vec = (t->d % 4 == 0 && aligned16(t->E, t->R)) ? 1 : 0;
    if (int rc = OKGE_TIMED("rows_gather", "rows_gather", st, launch_rows_gather(a, st))) return rc;
    okge_tables tv = *t;
    tv.E = a.EV; tv.R = a.RV; tv.n_ent = N + B; tv.n_rel = B;
    okge_prefix_batch vb = *batch;
    vb.po_obj = a.pos_ids; vb.sp_subj = a.pos_ids + batch->n_po;
    vb.po_rel = a.pos_ids + B; vb.sp_rel = a.pos_ids + B + batch->n_po;
    okge_candidates vc = *cand;
    vc.ids = nullptr; vc.first_id = 0;
    return train_core(&tv, nullptr, &vb, nullptr, 0, B, &vc, pos, loss_kind, label_smoothing, normalizer, N,
                      OKGE_TRAIN_GRADS_ZERO | OKGE_TRAIN_UNIQUE_CANDIDATES | OKGE_TRAIN_DISTINCT_PREFIX_ROWS, loss_out, dE, dR, nullptr,
                      scores, ld_scores, nullptr, workspace, train_total, stream);
}

// the local table of a sharded phase: tables, slot size (`unsharded`: the entry points that go on to 4096, as the message
// names them), shard range
int check_local_table(const okge_tables *t, const okge_shard *sh, const okge_candidates *cand, const char *unsharded)
{
    if (!t || !cand || !t->E || t->d <= 0 || t->n_ent <= 0) return fail(OKGE_ERR_INVALID, "bad tables");
    if (t->d > 512)
        return fail(OKGE_ERR_UNSUPPORTED, std::string("slot sizes above 512 are not supported by the tile kernels: the sharded phases stop "
                                                      "there, the unsharded ") + unsharded + " slot sizes up to 4096");
    return check_shard(t, sh);
}

int check_query_call(const okge_tables *t, const okge_shard *sh, const float *Q, int64_t ldq, int32_t B, const okge_candidates *cand)
{
    if (int rc = check_local_table(t, sh, cand, "okge_score_prefixes / okge_train_forward_backward take")) return rc;
    if (!Q || B <= 0 || cand->n <= 0 || ldq != okge_query_ld(t->d))
        return fail(OKGE_ERR_INVALID, "bad query block / candidates");
    if (cand->table) return fail(OKGE_ERR_INVALID, "sharded calls take candidates from the local entity table");
    return check_local_range(t, cand);
}

}  // namespace

extern "C" {

size_t okge_train_workspace_bytes(int32_t B, int32_t N, int32_t d)
{
    if (d > 512) {
        WideShape w;
        return make_wide_shape(B, N, d, w) ? wide_train_layout(w, plan_wide(w, read_knobs())).total : 0;
    }
    Shape s;
    if (!make_shape(B, N, d, s)) return 0;
    return train_layout(s, plan_train(s, cu_count(), read_knobs())).total;
}

size_t okge_score_workspace_bytes(int32_t B, int32_t d)
{
    if (d > 512) {
        WideShape w;
        return make_wide_shape(B, 1, d, w) ? wide_score_layout(w).total : 0;
    }
    Shape s;
    return make_shape(B, 1, d, s) ? score_layout(s).total : 0;
}

size_t okge_lse_workspace_bytes(int32_t B, int32_t N, int32_t d)
{
    if (d > 512) {
        WideShape w;
        return make_wide_shape(B, N, d, w) ? wide_train_layout(w, plan_wide(w, read_knobs())).lse_bytes : 0;
    }
    Shape s;
    if (!make_shape(B, N, d, s)) return 0;
    return lse_layout(s, plan_ranges(s, cu_count(), read_knobs())).lse_bytes;
}

int okge_score_prefixes(const okge_tables *t, const okge_prefix_batch *batch, const okge_candidates *cand,
                        float *scores, int64_t ld_scores, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = check_common(t, batch, cand, true)) return rc;
    if (!scores || ld_scores < cand->n) return fail(OKGE_ERR_INVALID, "bad scores buffer");
    if (is_wide(t->d)) return wide_score(t, batch, cand, scores, ld_scores, workspace, workspace_bytes, stream);
    Shape g;
    if (!make_shape(batch->n_po + batch->n_sp, cand->n, t->d, g)) return fail(OKGE_ERR_INVALID, "bad shape");
    const ScoreLayout l = score_layout(g);   // only the query block
    if (!workspace || workspace_bytes < l.total) return fail(OKGE_ERR_WORKSPACE, "workspace too small");
    hipStream_t st = as_stream(stream);
    float *Q = reinterpret_cast<float *>(static_cast<char *>(workspace) + l.off_Q);
    if (int rc = fold_for_sweep(t, batch, Q, g.ldq, g.Bpad, g.tiles, NT, st)) return rc;
    FusedArgs a;
    fill_fused_common(a, g, t, cand, Q);     // (all rows per workgroup: rows are independent in score mode, but one pass per tile keeps C resident)
    a.X = scores;
    a.ldx = ld_scores;
    a.x_vec_ok = x_vec_ok(scores, ld_scores);
    return OKGE_TIMED("fused_tile_score", "fused_tile_kernel<score>", st, launch_sweep(g, plan_sweep(g, g.tiles, cu_count(), read_knobs()), a, st));
}

size_t okge_train_row_grads_workspace_bytes(int32_t B, int32_t N, int32_t d)
{
    Shape s;
    if (d > 512 || !make_shape(B, N, d, s)) return 0;     // (the row-sparse step stops at slot size 512)
    return row_grads_layout(s, train_layout(s, plan_train(s, cu_count(), read_knobs())).total).total;
}

int okge_train_forward_backward(const okge_tables *t, const okge_prefix_batch *batch, const okge_candidates *cand,
                                const okge_positives *pos, int32_t loss_kind, float label_smoothing,
                                double normalizer, int32_t flags, double *loss_out, float *dE, float *dR,
                                float *scores, int64_t ld_scores, void *workspace, size_t workspace_bytes,
                                void *stream)
{
    if (int rc = check_common(t, batch, cand, true)) return rc;
    if (const int32_t frozen = flags & FREEZE_FLAGS) {       // (statuses first: nothing is launched, no output touched)
        if (frozen == FREEZE_FLAGS)
            return fail(OKGE_ERR_INVALID, "OKGE_TRAIN_FREEZE_ENTITIES and OKGE_TRAIN_FREEZE_RELATIONS together leave nothing to train");
        if (flags & OKGE_TRAIN_ROW_GRADS)
            return fail(OKGE_ERR_UNSUPPORTED, "OKGE_TRAIN_FREEZE_ENTITIES / OKGE_TRAIN_FREEZE_RELATIONS belong to the dense call of "
                                              "okge_train_forward_backward: not with OKGE_TRAIN_ROW_GRADS");
        if (int rc = refuse_bias(t->scorer, "okge_train_forward_backward(OKGE_TRAIN_FREEZE_*)", "the unused slot is already untouched")) return rc;
        if (flags & OKGE_TRAIN_LOSS_ONLY) flags &= ~FREEZE_FLAGS;                 // (no gradient either way)
        if (flags & OKGE_TRAIN_FREEZE_ENTITIES) dE = nullptr;                    // the frozen table's buffer is never looked at
        if (flags & OKGE_TRAIN_FREEZE_RELATIONS) dR = nullptr;
    }
    if (!(flags & (OKGE_TRAIN_LOSS_ONLY | OKGE_TRAIN_FREEZE_RELATIONS)) && !dR) return fail(OKGE_ERR_INVALID, "null output");
    if (is_wide(t->d)) {
        if (flags & OKGE_TRAIN_ROW_GRADS)
            return fail(OKGE_ERR_UNSUPPORTED, "OKGE_TRAIN_ROW_GRADS stops at slot size 512: slot sizes 513 to 4096 train with dense gradients");
        return wide_core(t, batch, cand, pos, loss_kind, label_smoothing, normalizer, flags, loss_out, dE, dR, scores, ld_scores,
                         workspace, workspace_bytes, stream);
    }
    if (flags & OKGE_TRAIN_ROW_GRADS)
        return train_row_grads(t, batch, cand, pos, loss_kind, label_smoothing, normalizer, flags, loss_out, dE, dR, scores, ld_scores,
                               workspace, workspace_bytes, stream);
    return train_core(t, nullptr, batch, nullptr, 0, batch->n_po + batch->n_sp, cand, pos, loss_kind, label_smoothing,
                      normalizer, cand->n, flags, loss_out, dE, dR, nullptr, scores, ld_scores, nullptr, workspace,
                      workspace_bytes, stream);
}

// ---- the N3 regulariser beside the step (okge_n3.hip; grid and workspace: plan_n3) --------------------------------
size_t okge_n3_workspace_bytes(int32_t B, int32_t N, int32_t d)
{
    N3Plan p;
    return plan_n3(B, N, d, p) ? p.total : 0;
}

int okge_n3_forward_backward(const okge_tables *t, const okge_prefix_batch *batch, const okge_candidates *cand, double coef,
                             int32_t cand_passes, double normalizer, int32_t flags, double *reg_out, float *dE, float *dR,
                             void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = check_common(t, batch, cand, true)) return rc;
    if (int rc = refuse_bias(t->scorer, "okge_n3_forward_backward", "the reference's l2_reg belongs to the lookup ComplEx / DistMult embedder")) return rc;
    if (cand->table) return fail(OKGE_ERR_INVALID, "the regulariser needs candidates from the entity table");
    if (cand_passes < 0 || cand_passes > 2) return fail(OKGE_ERR_INVALID, "cand_passes must be 0, 1 or 2");
    if (!(coef >= 0) || !(coef <= 3.0e38)) return fail(OKGE_ERR_INVALID, "coef must be a finite non-negative number");
    if (!(normalizer > 0)) return fail(OKGE_ERR_INVALID, "normalizer must be positive");
    const bool loss_only = (flags & OKGE_TRAIN_LOSS_ONLY) != 0, row_grads = (flags & OKGE_TRAIN_ROW_GRADS) != 0;
    if (!reg_out || (!loss_only && (!dE || !dR))) return fail(OKGE_ERR_INVALID, "null output");
    if (loss_only && row_grads) return fail(OKGE_ERR_INVALID, "OKGE_TRAIN_ROW_GRADS asks for gradients: not with OKGE_TRAIN_LOSS_ONLY");
    const int B = batch->n_po + batch->n_sp;
    N3Plan pl;
    if (!plan_n3(B, cand->n, t->d, pl)) return fail(OKGE_ERR_INVALID, "bad shape");
    if (!workspace || workspace_bytes < pl.total) return fail(OKGE_ERR_WORKSPACE, "workspace too small (okge_n3_workspace_bytes)");
    hipStream_t st = as_stream(stream);
    N3Args a;
    std::memset(&a, 0, sizeof(a));
    a.E = t->E; a.R = t->R;
    a.dE = loss_only ? nullptr : dE; a.dR = loss_only ? nullptr : dR;
    a.partial = static_cast<double *>(workspace);
    a.cand_ids = cand->ids; a.cand_first = cand->first_id; a.N = cand->n;
    a.p = to_dev(*batch, t);
    a.drop_c = to_dev(cand->drop);
    a.value_cand = coef * cand_passes; a.value_prefix = coef;
    a.grad_cand = 3.0 * coef * cand_passes / normalizer; a.grad_prefix = 3.0 * coef / normalizer;
    a.n_ent = t->n_ent; a.d = t->d; a.n_oct = pl.n_oct; a.rows_per_wg = pl.rows_per_wg;
    a.cand_wgs = cand_passes ? pl.cand_wgs : 0;
    a.vec = (t->d % 4 == 0 && aligned16(t->E, t->R) && (loss_only || aligned16(dE, dR))) ? 1 : 0;
    a.loss_only = loss_only ? 1 : 0;
    a.row_grads = row_grads ? 1 : 0;
    // one lane owns every element it adds to -- a candidate range, a list the caller vouches for, distinct prefix rows,
    // occurrence rows -- or an id may repeat: float atomics
    a.cand_atomic = (row_grads || !cand->ids || (flags & OKGE_TRAIN_UNIQUE_CANDIDATES)) ? 0 : 1;
    a.prefix_atomic = (row_grads || (flags & OKGE_TRAIN_DISTINCT_PREFIX_ROWS)) ? 0 : 1;
    // a prefix entity may be a candidate: plain candidate updates and atomic prefix updates of one row must not meet in a launch
    const int n_wgs = a.cand_wgs + pl.prefix_wgs, first = (!loss_only && !a.cand_atomic && a.prefix_atomic) ? a.cand_wgs : n_wgs;
    if (int rc = OKGE_TIMED("n3", "n3_kernel", st, launch_n3(a, 0, first, st))) return rc;
    if (int rc = OKGE_TIMED("n3", "n3_kernel", st, launch_n3(a, first, n_wgs - first, st))) return rc;
    return OKGE_TIMED("loss_reduce", "loss_reduce", st, launch_loss_reduce(a.partial, a.cand_wgs + pl.prefix_wgs, reg_out, st));
}

// ---- entity-sharded phases ---------------------------------------------------------------------------------------
int64_t okge_query_ld(int32_t d)
{
    Shape s;
    return make_shape(1, 1, d, s) ? s.ldq : 0;
}

int32_t okge_query_rows(int32_t B)
{
    Shape s;
    return make_shape(B, 1, 1, s) ? s.Bpad : 0;
}

int okge_encode_queries(const okge_tables *t, const okge_shard *sh, const okge_prefix_batch *batch, float *Q,
                        int64_t ldq, float *ent_rows, void *stream)
{
    if (int rc = check_common(t, batch)) return rc;
    if (int rc = check_shard(t, sh)) return rc;
    if ((!Q && !ent_rows) || ldq != okge_query_ld(t->d)) return fail(OKGE_ERR_INVALID, "bad query block");
    hipStream_t st = as_stream(stream);
    const PrefixDev p = to_dev(*batch, t, sh);
    return OKGE_TIMED("encode_queries", "encode_queries", st,
                      launch_encode_queries(t->E, t->R, t->d, t->scorer, p, Q, (int)ldq, okge_query_rows(batch->n_po + batch->n_sp), ent_rows,
                                            nullptr, 0, nullptr, 0, NT, 0, st));
}

int okge_fold_queries(const okge_tables *t, const okge_prefix_batch *batch, const float *ent_rows, int64_t ldq, float *Q,
                      void *stream)
{
    if (int rc = check_common(t, batch)) return rc;
    if (int rc = refuse_bias(t->scorer, "okge_fold_queries", "the sharded paths are not built for it")) return rc;
    if (!ent_rows || !Q || ldq != okge_query_ld(t->d)) return fail(OKGE_ERR_INVALID, "bad query block");
    hipStream_t st = as_stream(stream);
    PrefixDev p = to_dev(*batch, t);
    p.ent_lo = 0; p.ent_hi = 0x7fffffff; p.whole_table = 0;     // entity ids are global here and not dereferenced: only relations are
    return OKGE_TIMED("fold_queries", "fold_queries", st,
                      launch_fold_queries(t->R, t->d, t->scorer, p, ent_rows, Q, (int)ldq, okge_query_rows(batch->n_po + batch->n_sp), st));
}

int okge_train_tiles(const okge_tables *t, const okge_shard *sh, const float *Q, int64_t ldq, int32_t B,
                     const okge_candidates *cand, const okge_positives *pos, int32_t loss_kind, float label_smoothing,
                     double normalizer, int32_t n_cand_global, int32_t flags, const float *row_lse, double *loss_out,
                     float *dE, float *dQ, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = check_local_table(t, sh, cand, "okge_train_forward_backward takes")) return rc;
    if (!Q || !dQ || B <= 0 || cand->n <= 0) return fail(OKGE_ERR_INVALID, "bad query block / candidates");
    if (int rc = check_local_range(t, cand)) return rc;
    return train_core(t, sh, nullptr, Q, ldq, B, cand, pos, loss_kind, label_smoothing, normalizer, n_cand_global,
                      flags & ~FREEZE_FLAGS, loss_out, dE, nullptr, dQ, nullptr, 0, row_lse, workspace, workspace_bytes, stream);
}

int okge_score_queries(const okge_tables *t, const okge_shard *sh, const float *Q, int64_t ldq, int32_t B,
                       const okge_candidates *cand, float *scores, int64_t ld_scores, void *stream)
{
    if (int rc = check_query_call(t, sh, Q, ldq, B, cand)) return rc;
    if (!scores || ld_scores < cand->n) return fail(OKGE_ERR_INVALID, "bad scores buffer");
    Shape g;
    if (!make_shape(B, cand->n, t->d, g)) return fail(OKGE_ERR_INVALID, "bad shape");
    hipStream_t st = as_stream(stream);
    FusedArgs a;
    fill_fused_common(a, g, t, cand, Q);
    a.cand_col0 = sh->cand_col0;
    a.X = scores;
    a.ldx = ld_scores;
    a.x_vec_ok = x_vec_ok(scores, ld_scores);
    return OKGE_TIMED("fused_tile_score", "fused_tile_kernel<score>", st, launch_sweep(g, plan_sweep(g, g.tiles, cu_count(), read_knobs()), a, st));
}

int okge_row_logsumexp(const okge_tables *t, const okge_shard *sh, const float *Q, int64_t ldq, int32_t B,
                       const okge_candidates *cand, float *row_lse, void *workspace, size_t workspace_bytes,
                       void *stream)
{
    if (int rc = check_query_call(t, sh, Q, ldq, B, cand)) return rc;
    if (!row_lse) return fail(OKGE_ERR_INVALID, "null output");
    Shape g;
    if (!make_shape(B, cand->n, t->d, g)) return fail(OKGE_ERR_INVALID, "bad shape");
    const SweepCtx cx = {g, cu_count(), read_knobs()};
    const Ranges rg = plan_ranges(g, cx.cus, cx.knobs);
    const LseLayout l = lse_layout(g, rg);
    if (!workspace || workspace_bytes < l.lse_bytes) return fail(OKGE_ERR_WORKSPACE, "workspace too small");
    FusedArgs a;
    fill_fused_common(a, g, t, cand, Q);
    a.cand_col0 = sh->cand_col0;
    return lse_pass(cx, rg, l, a, static_cast<char *>(workspace), row_lse, as_stream(stream));
}

size_t okge_topk_workspace_bytes(int32_t B, int32_t N, int32_t d, int32_t k, int32_t range_n)
{
    Shape s;
    TopkPlan tp;
    return make_shape(B, N, d, s) && plan_topk(s, k, range_n, cu_count(), tp) ? tp.total : 0;
}

int okge_topk_prefixes(const okge_tables *t, const okge_prefix_batch *batch, const okge_candidates *cand, int32_t k,
                       const int64_t *filt_ptr, const int32_t *filt_col, int64_t n_filter, int32_t range_n, float *out_scores,
                       int32_t *out_cols, int32_t *out_ids, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = check_common(t, batch, cand)) return rc;
    if (int rc = refuse_bias(t->scorer, "okge_topk_prefixes", "predictions are built for the ComplEx and DistMult scorers")) return rc;
    if (int rc = check_topk(k, batch, cand, filt_ptr, filt_col, n_filter, range_n, out_scores, out_cols)) return rc;
    if (!out_ids) return fail(OKGE_ERR_INVALID, "null output");
    Shape g;
    if (!make_shape(batch->n_po + batch->n_sp, cand->n, t->d, g)) return fail(OKGE_ERR_INVALID, "bad shape");
    const SweepCtx cx = {g, cu_count(), read_knobs()};
    TopkPlan tp;
    if (!plan_topk(g, k, range_n, cx.cus, tp)) return fail(OKGE_ERR_INVALID, "bad shape");
    if (!workspace || workspace_bytes < tp.total) return fail(OKGE_ERR_WORKSPACE, "workspace too small");
    hipStream_t st = as_stream(stream);
    char *ws = static_cast<char *>(workspace);
    float *Q = reinterpret_cast<float *>(ws + tp.off_Q);
    if (int rc = fold_for_sweep(t, batch, Q, g.ldq, g.Bpad, g.tiles, NT, st)) return rc;
    FusedArgs a;
    fill_fused_common(a, g, t, cand, Q);
    return topk_pass(cx, tp, a, ws, k, n_filter > 0 ? filt_ptr : nullptr, filt_col, out_scores, out_cols, out_ids, st);
}

int okge_topk_queries(const okge_tables *t, const okge_shard *sh, const float *Q, int64_t ldq, int32_t B,
                      const okge_candidates *cand, int32_t k, const int64_t *filt_ptr, const int32_t *filt_col, int64_t n_filter,
                      int32_t range_n, float *out_scores, int32_t *out_cols, void *workspace, size_t workspace_bytes, void *stream)
{
    if (cand && cand->table) return fail(OKGE_ERR_UNSUPPORTED, "top-k takes its candidates from the entity table");
    if (int rc = check_query_call(t, sh, Q, ldq, B, cand)) return rc;
    if (int rc = check_topk(k, nullptr, cand, filt_ptr, filt_col, n_filter, range_n, out_scores, out_cols)) return rc;
    Shape g;
    if (!make_shape(B, cand->n, t->d, g)) return fail(OKGE_ERR_INVALID, "bad shape");
    const SweepCtx cx = {g, cu_count(), read_knobs()};
    TopkPlan tp;
    if (!plan_topk(g, k, range_n, cx.cus, tp)) return fail(OKGE_ERR_INVALID, "bad shape");
    if (!workspace || workspace_bytes < tp.total) return fail(OKGE_ERR_WORKSPACE, "workspace too small");
    FusedArgs a;
    fill_fused_common(a, g, t, cand, Q);
    a.cand_col0 = sh->cand_col0;
    return topk_pass(cx, tp, a, static_cast<char *>(workspace), k, n_filter > 0 ? filt_ptr : nullptr, filt_col, out_scores, out_cols, nullptr,
                     as_stream(stream));
}

int okge_topk_merge(const float *scores, const int32_t *cols, int32_t n_lists, int32_t B, int32_t k, float *out_scores,
                    int32_t *out_cols, void *stream)
{
    if (!scores || !cols || !out_scores || !out_cols || n_lists <= 0 || B <= 0) return fail(OKGE_ERR_INVALID, "bad lists");
    if (int rc = check_topk_k(k)) return rc;
    hipStream_t st = as_stream(stream);
    TopkMergeArgs m;
    std::memset(&m, 0, sizeof(m));
    m.sc = scores; m.cl = cols; m.elem_stride = 1;
    m.L = n_lists; m.rows_ld = B; m.kq = k; m.B = B; m.k = k;
    m.first = 1;
    m.out_sc = out_scores; m.out_cl = out_cols;
    return OKGE_TIMED("topk_merge", "topk_merge", st, launch_topk_merge(m, st));
}

int okge_prefix_backward(const okge_tables *t, const okge_shard *sh, const okge_prefix_batch *batch, const float *dQ,
                         int64_t ldq, const float *ent_rows, float *dE, float *dR, void *stream)
{
    if (int rc = check_common(t, batch)) return rc;
    if (int rc = check_shard(t, sh)) return rc;
    if (!dQ || !dE || !dR || ldq != okge_query_ld(t->d)) return fail(OKGE_ERR_INVALID, "bad prefix_backward arguments");
    hipStream_t st = as_stream(stream);
    const PrefixDev p = to_dev(*batch, t, sh);
    const int B = batch->n_po + batch->n_sp;
    return OKGE_TIMED("prefix_backward", "prefix_backward", st,
                      launch_prefix_backward(t->E, t->R, t->d, t->scorer, p, dQ, 1, okge_query_rows(B), (int)ldq, ent_rows, dE, dR, nullptr, 0,
                                             nullptr, st));
}

int okge_prefix_backward_segmented(const okge_tables *t, const okge_shard *sh, const okge_prefix_batch *batch, const float *dQ,
                                   int64_t ldq, const float *ent_rows, const int32_t *rel_order, const int32_t *rel_seg_ptr,
                                   int32_t n_rel_seg, const int32_t *ent_order, const int32_t *ent_seg_ptr, int32_t n_ent_seg,
                                   float *grad_rows, float *dE, float *dR, void *stream)
{
    if (int rc = check_common(t, batch)) return rc;
    if (int rc = check_shard(t, sh)) return rc;
    if (!dQ || !dE || !dR || ldq != okge_query_ld(t->d)) return fail(OKGE_ERR_INVALID, "bad prefix_backward arguments");
    const int B = batch->n_po + batch->n_sp;
    const bool has_r = rel_order || rel_seg_ptr || n_rel_seg, has_e = ent_order || ent_seg_ptr || n_ent_seg;
    if (!grad_rows || (!has_r && !has_e) || (has_r && (!rel_order || !rel_seg_ptr || n_rel_seg <= 0 || n_rel_seg > B)) ||
        (has_e && (!ent_order || !ent_seg_ptr || n_ent_seg <= 0 || n_ent_seg > B)))
        return fail(OKGE_ERR_INVALID, "bad row segments (order[B], seg_ptr[n_seg + 1], 1 <= n_seg <= B; grad_rows[2][rows][ldq])");
    const bool vec = t->scorer == OKGE_COMPLEX ? (t->d % 8 == 0) : (t->d % 4 == 0);
    if (!vec) return fail(OKGE_ERR_UNSUPPORTED, "segmented gradients need d % 8 == 0 (ComplEx) / d % 4 == 0 (DistMult, data-bias)");
    hipStream_t st = as_stream(stream);
    const PrefixDev p = to_dev(*batch, t, sh);
    return OKGE_TIMED("prefix_backward", "prefix_backward_segmented", st,
                      launch_prefix_backward(t->E, t->R, t->d, t->scorer, p, dQ, 1, okge_query_rows(B), (int)ldq, ent_rows, dE, dR, nullptr, 0,
                                             nullptr, st, rel_order, rel_seg_ptr, n_rel_seg, ent_order, ent_seg_ptr, n_ent_seg, grad_rows));
}

}  // extern "C"
