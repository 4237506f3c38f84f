// C ABI (include/okge.h) over the gfx950 kernels.  Host-side only: argument checking, workspace carving,
// launch geometry, HIP-event timing.  No torch, no CPU fallback: every entry point either enqueues HIP
// kernels or returns an error.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/okge.h"
#include "okge_kernels.h"
#include "okge_plan.h"
#include "okge_wide.h"

using namespace okge;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

int fail_hip(hipError_t e, const char *what)
{
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    return OKGE_ERR_HIP;
}

// ---- per-kernel HIP-event timing ----------------------------------------------------------------------
struct TimedLaunch {
    const char *name;
    hipEvent_t  start, stop;
};
std::mutex               g_tmu;
bool                     g_timing = false;
std::vector<TimedLaunch> g_launches;
std::vector<hipEvent_t>  g_event_pool;

hipEvent_t get_event()
{
    if (!g_event_pool.empty()) {
        hipEvent_t e = g_event_pool.back();
        g_event_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}

struct ScopedTimer {
    hipStream_t st;
    bool        on;
    TimedLaunch t;
    ScopedTimer(const char *name, hipStream_t s) : st(s), on(g_timing)
    {
        if (!on) return;
        std::lock_guard<std::mutex> lk(g_tmu);
        t.name = name;
        t.start = get_event();
        t.stop = get_event();
        (void)hipEventRecord(t.start, st);
    }
    ~ScopedTimer()
    {
        if (!on) return;
        (void)hipEventRecord(t.stop, st);
        std::lock_guard<std::mutex> lk(g_tmu);
        g_launches.push_back(t);
    }
};

// ---- device word counting out-of-range ids (checked_row in the kernels); read and cleared by okge_id_errors ------------
// One word PER DEVICE (keyed by hipGetDevice() at the call): a process that drives several devices must never hand a kernel
// on device b a pointer that lives on device a.
constexpr int OKGE_MAX_DEVICES = 64;
static std::mutex g_dev_mu;
static int *g_id_err[OKGE_MAX_DEVICES] = {};
int current_device()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= OKGE_MAX_DEVICES) return -1;
    return dev;
}
int *id_err_ptr()
{
    const int dev = current_device();
    if (dev < 0) return nullptr;
    std::lock_guard<std::mutex> lk(g_dev_mu);
    if (!g_id_err[dev]) {
        if (hipMalloc(reinterpret_cast<void **>(&g_id_err[dev]), sizeof(int)) != hipSuccess) { g_id_err[dev] = nullptr; return nullptr; }
        (void)hipMemset(g_id_err[dev], 0, sizeof(int));
    }
    return g_id_err[dev];
}

// ---- helpers ---------------------------------------------------------------------------------------------
DropDev to_dev(const okge_dropout &d)
{
    DropDev r;
    std::memset(&r, 0, sizeof(r));
    r.scale = 1.f;
    if (d.p > 0.f) {
        r.enabled = 1;
        r.keep = d.keep;
        r.scale = 1.0f / (1.0f - d.p);
        const double t = (double)d.p * 65536.0;
        r.thr = t <= 0 ? 0u : (t >= 65535.0 ? 65535u : (uint32_t)t);
        r.k0 = (uint32_t)d.seed;
        r.k1 = (uint32_t)(d.seed >> 32);
        r.stream = d.stream;
        r.step = d.step;
        r.step_dev = d.step_dev;
    }
    return r;
}

PrefixDev to_dev(const okge_prefix_batch &b, const okge_tables *t, const okge_shard *sh = nullptr)
{
    PrefixDev p;
    p.po_rel = b.po_rel; p.po_obj = b.po_obj; p.sp_subj = b.sp_subj; p.sp_rel = b.sp_rel;
    p.n_po = b.n_po; p.n_sp = b.n_sp;
    p.ent_lo = sh ? sh->ent_lo : 0;
    p.ent_hi = sh ? sh->ent_hi : t->n_ent;          // unsharded: the range IS the table, an id outside it is an error
    p.whole_table = sh ? 0 : 1;
    p.n_rel = t->n_rel;
    p.id_err = id_err_ptr();
    p.drop_po_ent = to_dev(b.drop_po_ent); p.drop_po_rel = to_dev(b.drop_po_rel);
    p.drop_sp_ent = to_dev(b.drop_sp_ent); p.drop_sp_rel = to_dev(b.drop_sp_rel);
    return p;
}

static_assert(sizeof(v8bf) == PLANE_CELL_BYTES && sizeof(TopkRec) == TOPK_REC_BYTES, "okge_plan.h sizes its regions with these");

// compute units of the current device (stream-K launches: one workgroup per CU); 256 where no device answers.  The planner
// (okge_plan.h) takes it as an argument.
int cu_count()
{
    static std::mutex mu;
    static int cus[OKGE_MAX_DEVICES] = {};
    const int dev = current_device();
    if (dev < 0) return 256;
    std::lock_guard<std::mutex> lk(mu);
    if (!cus[dev]) {
        int n = 0;
        cus[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
    }
    return cus[dev];
}

bool known_scorer(int32_t scorer)
{
    return scorer == OKGE_COMPLEX || scorer == OKGE_DISTMULT || scorer == OKGE_BIAS_RELATION || scorer == OKGE_BIAS_ENTITY;
}
const char *scorer_name(int32_t scorer) { return scorer == OKGE_BIAS_RELATION ? "OKGE_BIAS_RELATION" : "OKGE_BIAS_ENTITY"; }
// the data-bias scorers (model.py:281-350) score prefixes only and leave one slot without a gradient: the entry points that
// score triples, step every table or fold from exchanged entity rows refuse them before anything is written
int refuse_bias(int32_t scorer, const char *entry, const char *why)
{
    if (scorer != OKGE_BIAS_RELATION && scorer != OKGE_BIAS_ENTITY) return OKGE_OK;
    return fail(OKGE_ERR_UNSUPPORTED, std::string(entry) + " does not take the " + scorer_name(scorer) + " scorer: " + why);
}

// wide_ok: the entry point has a wide path (slot sizes 513 .. 4096: okge_score_prefixes, okge_train_forward_backward,
// okge_evaluate_batch); every other one stops at 512
int check_common(const okge_tables *t, const okge_prefix_batch *b, const okge_candidates *c, bool wide_ok = false)
{
    if (!t || !b || !c) return fail(OKGE_ERR_INVALID, "null descriptor");
    if (!t->E || !t->R) return fail(OKGE_ERR_INVALID, "null embedding table");
    if (t->d <= 0 || t->n_ent <= 0 || t->n_rel <= 0) return fail(OKGE_ERR_INVALID, "bad table shape");
    if (!known_scorer(t->scorer)) return fail(OKGE_ERR_INVALID, "unknown scorer");
    if (t->scorer == OKGE_COMPLEX && (t->d & 1)) return fail(OKGE_ERR_INVALID, "ComplEx needs an even slot size");
    if (t->d > WIDE_MAX_D) return fail(OKGE_ERR_UNSUPPORTED, "slot sizes above 4096 are not supported");
    if (t->d > 512 && !wide_ok)
        return fail(OKGE_ERR_UNSUPPORTED, "slot sizes above 512 are not supported by the tile kernels: slot sizes 513 to 4096 run through "
                                          "okge_score_prefixes, okge_train_forward_backward (dense gradients) and okge_evaluate_batch");
    if (t->d > 512 && sc_is_bias(t->scorer))
        return fail(OKGE_ERR_UNSUPPORTED, "the data-bias scorers stop at slot size 512: the wide path is built for ComplEx and DistMult");
    if (b->n_po < 0 || b->n_sp < 0 || b->n_po + b->n_sp <= 0) return fail(OKGE_ERR_INVALID, "empty batch");
    if (b->n_po > 0 && (!b->po_rel || !b->po_obj)) return fail(OKGE_ERR_INVALID, "null po ids");
    if (b->n_sp > 0 && (!b->sp_subj || !b->sp_rel)) return fail(OKGE_ERR_INVALID, "null sp ids");
    if (c->n <= 0) return fail(OKGE_ERR_INVALID, "no candidates");
    const int64_t cand_rows = c->table ? c->table_rows : t->n_ent;
    if (!c->ids && (c->first_id < 0 || (int64_t)c->first_id + c->n > cand_rows))
        return fail(OKGE_ERR_INVALID, "candidate range outside the candidate table");
    return OKGE_OK;
}

// the arguments every tile launch shares; Q: the folded queries.  b_per_block: all rows (the sweeps; train_core sets its split)
void fill_fused_common(FusedArgs &a, const Shape &s, const okge_tables *t, const okge_candidates *c, const float *Q)
{
    std::memset(&a, 0, sizeof(a));
    a.E = c->table ? c->table : t->E;       // table the candidate rows are gathered from
    a.n_table_rows = c->table ? c->table_rows : t->n_ent;
    a.id_err = id_err_ptr();
    a.cand_ids = c->ids;
    a.cand_first = c->first_id;
    a.Q = Q;
    a.drop_c = to_dev(c->drop);
    a.d = s.d; a.KB = s.KB; a.LDK = s.LDK; a.N = s.N; a.B = s.B; a.Bpad = s.Bpad; a.ldq = s.ldq;
    a.b_per_block = s.Bpad;
}


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

// the score sweep (MODE_SCORE / _STATS / _COUNT / _TOPK) of p.tiles 64-candidate tiles over all B rows, as plan_sweep cut it:
// the 64 x 64 kernel up to slot size 256 (rows are independent: the tail tiles simply run as (tile, row split) workgroups);
// above, the register-tile kernel in a stream-K launch (no partial outputs to add up)
hipError_t launch_sweep(const Shape &s, const SweepPlan &p, const FusedArgs &a0, hipStream_t st, int mode = MODE_SCORE)
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

// what a sweep needs beside its arguments: the shape and what the planner reads
struct SweepCtx {
    const Shape &s;
    int          cus;
    Knobs        knobs;
    SweepPlan    plan(int tiles) const { return plan_sweep(s, tiles, cus, knobs); }
};

// Arguments of candidate range r (ranges of rg.range_n candidates): local candidate 0 of the launch is
// candidate r * range_n of the call.  Positives / dropout keep their global columns through cand_col0.
// loss_stride: loss partials per tile of the launch that owns base.loss_partial (the train plan's b_split)
FusedArgs range_args(const FusedArgs &base, const Shape &s, const Ranges &rg, int r, int &tiles_r, int loss_stride = 1)
{
    FusedArgs a = base;
    const int n_lo = r * rg.range_n;
    a.N = std::min(rg.range_n, s.N - n_lo);
    a.cand_first += n_lo;
    if (a.cand_ids) a.cand_ids += n_lo;
    a.cand_col0 += n_lo;
    if (a.tile_ptr) a.tile_ptr += n_lo / NT;
    if (a.loss_partial) a.loss_partial += (size_t)(n_lo / NT) * loss_stride;
    tiles_r = (a.N + NT - 1) / NT;
    return a;
}

// per-row log-sum-exp over all candidates of the call (KL loss): one score-statistics pass per candidate range, merged
// into a running (max, sum-exp) per row; the (B, N) scores are never materialised
int lse_pass(const SweepCtx &cx, const Ranges &rg, const LseLayout &l, const FusedArgs &base, char *ws, float *row_lse, hipStream_t st,
             const int32_t *count_pos_row = nullptr, int count_nnz = 0, float *count_ysum = nullptr)
{
    const Shape &g = cx.s;
    FusedArgs b = base;
    b.stats = reinterpret_cast<float *>(ws + l.off_stats);
    b.b_per_block = g.Bpad;
    b.tile_ptr = nullptr;
    b.loss_partial = nullptr;
    for (int r = 0; r < rg.n_ranges; ++r) {
        int tiles_r;
        const FusedArgs s = range_args(b, g, rg, r, tiles_r);
        hipError_t e;
        {
            ScopedTimer tm("fused_tile_stats", st);
            e = launch_sweep(g, cx.plan(tiles_r), s, st, MODE_STATS);      // (slot sizes above 256: four 16-candidate blocks per tile)
            if (e != hipSuccess) return fail_hip(e, "fused_tile_kernel<stats>");
        }
        ScopedTimer tm("kl_row_lse", st);
        // the 64x64 cut emits one (max, sum-exp) per 64-candidate tile, the register-tile kernel one per 16-candidate block
        e = launch_kl_row_lse(s.stats, g.KB <= 16 ? tiles_r : 4 * tiles_r, g.B, g.Bpad,
                              reinterpret_cast<float *>(ws + l.off_run), r == 0, r == rg.n_ranges - 1, row_lse, st,
                              r == 0 ? count_pos_row : nullptr, count_nnz, r == 0 ? count_ysum : nullptr);   // + the rows' label mass
        if (e != hipSuccess) return fail_hip(e, "kl_row_lse");
    }
    return OKGE_OK;
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
        int tiles_r;
        FusedArgs s = range_args(b, g, tp, r, tiles_r);
        const SweepPlan sp = cx.plan(tiles_r);
        hipError_t e;
        if (g.KB <= 16) {
            s.tk_part = part;
            // (the name tells whether the closing round of this range was launched apart)
            ScopedTimer tm(sp.tail_split > 1 ? "fused_tile_topk_tail" : "fused_tile_topk", st);
            e = launch_sweep(g, sp, s, st, MODE_TOPK);
            if (e != hipSuccess) return fail_hip(e, "fused_tile_kernel<topk>");
        } else {
            s.X = reinterpret_cast<float *>(ws + tp.off_X);
            s.ldx = tp.range_n;
            {
                ScopedTimer tm("fused_tile_score", st);
                e = launch_sweep(g, sp, s, st, MODE_SCORE);
                if (e != hipSuccess) return fail_hip(e, "fused_tile64k_kernel<score>");
            }
            ScopedTimer tm("topk_cut", st);
            e = launch_topk_cut(s.X, s.ldx, g.B, g.Bpad, s.N, s.cand_col0, filt_ptr, filt_col, k, part, st);
            if (e != hipSuccess) return fail_hip(e, "topk_cut");
        }
        ScopedTimer tm("topk_merge", st);
        TopkMergeArgs m;
        std::memset(&m, 0, sizeof(m));
        m.sc = &part->score; m.cl = &part->col; m.elem_stride = 2;
        m.L = tiles_r; m.rows_ld = g.Bpad; m.kq = k; m.B = g.B; m.k = k;
        m.first = r == 0;
        m.out_sc = out_scores; m.out_cl = out_cols;
        if (r == tp.n_ranges - 1 && out_ids) { m.out_id = out_ids; m.cand_ids = base.cand_ids; m.cand_first = base.cand_first; }
        e = launch_topk_merge(m, st);
        if (e != hipSuccess) return fail_hip(e, "topk_merge");
    }
    return OKGE_OK;
}

bool any_dropout(const okge_prefix_batch *b, const okge_candidates *c)
{
    return c->drop.p > 0.f || (b && (b->drop_po_ent.p > 0.f || b->drop_po_rel.p > 0.f || b->drop_sp_ent.p > 0.f || b->drop_sp_rel.p > 0.f));
}

int check_topk(int32_t k, const okge_prefix_batch *b, const okge_candidates *c, const int64_t *filt_ptr, const int32_t *filt_col,
               int64_t n_filter, int32_t range_n, const float *out_scores, const int32_t *out_cols)
{
    if (k < 1) return fail(OKGE_ERR_INVALID, "k must be at least 1");
    if (k > 64) return fail(OKGE_ERR_UNSUPPORTED, "top-k keeps at most 64 candidates per row");
    if (c->table) return fail(OKGE_ERR_UNSUPPORTED, "top-k takes its candidates from the entity table");
    if (any_dropout(b, c)) return fail(OKGE_ERR_UNSUPPORTED, "top-k is an eval-mode call: no dropout");
    if (range_n < 0 || n_filter < 0 || (n_filter > 0 && (!filt_ptr || !filt_col))) return fail(OKGE_ERR_INVALID, "bad filter / range");
    if (!out_scores || !out_cols) return fail(OKGE_ERR_INVALID, "null output");
    return OKGE_OK;
}

// ---- the wide path: slot sizes 513 .. 4096 (okge_wide.hip; shapes, plan and layouts: okge_plan.h) ---------------------------
// the arguments every wide tile launch shares
void fill_wide_common(FusedArgs &a, const WideShape &s, const okge_tables *t, const okge_candidates *c, const float *Q)
{
    std::memset(&a, 0, sizeof(a));
    a.E = c->table ? c->table : t->E;
    a.n_table_rows = c->table ? c->table_rows : t->n_ent;
    a.id_err = id_err_ptr();
    a.cand_ids = c->ids;
    a.cand_first = c->first_id;
    a.Q = Q;
    a.drop_c = to_dev(c->drop);
    a.d = s.d; a.N = s.N; a.B = s.B; a.Bpad = s.Bpad; a.ldq = s.ldq;
    a.b_per_block = s.Bpad;
}

// arguments of the candidates [n_lo, n_lo + n) of the call (n_lo a multiple of the tile width): local candidate 0 of the
// launch is candidate n_lo of the call; positives and dropout keep their global columns through cand_col0
FusedArgs wide_range_args(const FusedArgs &base, const WideShape &s, int n_lo, int n)
{
    FusedArgs a = base;
    a.N = n;
    a.cand_first += n_lo;
    if (a.cand_ids) a.cand_ids += n_lo;
    a.cand_col0 += n_lo;
    if (a.tile_ptr) a.tile_ptr += n_lo / WIDE_TN;
    if (a.loss_partial) a.loss_partial += (size_t)(n_lo / WIDE_TN) * s.row_blocks;
    return a;
}

int wide_score(const okge_tables *t, const okge_prefix_batch *batch, const okge_candidates *cand, float *scores, int64_t ld_scores,
               void *workspace, size_t workspace_bytes, void *stream)
{
    WideShape g;
    if (!make_wide_shape(batch->n_po + batch->n_sp, cand->n, t->d, g)) return fail(OKGE_ERR_INVALID, "bad shape");
    const WideScoreLayout l = wide_score_layout(g);
    if (!workspace || workspace_bytes < l.total) return fail(OKGE_ERR_WORKSPACE, "workspace too small");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float *Q = reinterpret_cast<float *>(static_cast<char *>(workspace) + l.off_Q);
    const PrefixDev p = to_dev(*batch, t);
    {
        ScopedTimer tm("encode_queries", st);
        hipError_t e = launch_encode_queries(t->E, t->R, t->d, t->scorer, p, Q, g.ldq, g.Bpad, nullptr, nullptr, 0, nullptr, g.tiles,
                                             WIDE_TN, 0, st);
        if (e != hipSuccess) return fail_hip(e, "encode_queries");
    }
    FusedArgs a;
    fill_wide_common(a, g, t, cand, Q);
    a.X = scores;
    a.ldx = ld_scores;
    // (grid.y carries the tiles: sweep the candidates in launches of at most 32768 tiles)
    constexpr int MAX_TILES = 32768;
    for (int t0 = 0; t0 < g.tiles; t0 += MAX_TILES) {
        FusedArgs s = wide_range_args(a, g, t0 * WIDE_TN, std::min(g.N - t0 * WIDE_TN, MAX_TILES * WIDE_TN));
        s.X = scores + (size_t)t0 * WIDE_TN;
        ScopedTimer tm("wide_tile_score", st);
        hipError_t e = launch_wide_tile(MODE_SCORE, s, g.row_blocks, std::min(g.tiles - t0, MAX_TILES), st);
        if (e != hipSuccess) return fail_hip(e, "wide_tile_kernel<score>");
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
    if (!pos || pos->nnz < 0 || (pos->nnz > 0 && (!pos->col || !pos->row))) return fail(OKGE_ERR_INVALID, "bad positives");
    if (loss_kind != OKGE_LOSS_BCE && loss_kind != OKGE_LOSS_KL) return fail(OKGE_ERR_INVALID, "unknown loss");
    const bool loss_only = (flags & OKGE_TRAIN_LOSS_ONLY) != 0;
    if (!loss_out || (!loss_only && !dE)) return fail(OKGE_ERR_INVALID, "null output");
    if (cand->table) return fail(OKGE_ERR_INVALID, "training needs candidates from the entity table");
    if (!(normalizer > 0)) return fail(OKGE_ERR_INVALID, "normalizer must be positive");
    if (scores && ld_scores < cand->n) return fail(OKGE_ERR_INVALID, "bad scores buffer");
    const int B = batch->n_po + batch->n_sp;
    WideShape g;
    if (!make_wide_shape(B, cand->n, t->d, g)) return fail(OKGE_ERR_INVALID, "bad shape");
    const WidePlan pl = plan_wide(g, read_knobs());
    const WideTrainLayout l = wide_train_layout(g, pl);
    if (!workspace || workspace_bytes < l.total) return fail(OKGE_ERR_WORKSPACE, "workspace too small");
    if (pl.range_tiles > 65535) return fail(OKGE_ERR_UNSUPPORTED, "candidate range too long for one launch: lower OKGE_GT_MBYTES");
    const bool clear_grads = (flags & OKGE_TRAIN_CLEAR_GRADS) != 0 && !loss_only;
    if (clear_grads) {
        if (cand->ids || !dR) return fail(OKGE_ERR_INVALID, "OKGE_TRAIN_CLEAR_GRADS needs a contiguous candidate range on an unsharded table");
        flags |= OKGE_TRAIN_GRADS_ZERO;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace);
    float *Q = reinterpret_cast<float *>(ws + l.off_Q);
    const bool kl = loss_kind == OKGE_LOSS_KL;
    hipError_t e;
    {
        // folded queries + per-tile offsets into the column-sorted positives + the clears (see train_core: no memset nodes)
        ScopedTimer tm("encode_queries", st);
        const PrefixDev p = to_dev(*batch, t);
        ClearSpec clr = {};
        if (kl) { clr.p[3] = reinterpret_cast<float *>(ws + l.off_ysum); clr.n[3] = g.Bpad; }
        if (clear_grads) {
            const int64_t d64 = t->d, hi = (int64_t)cand->first_id + cand->n;
            clr.p[0] = dR;                      clr.n[0] = (int64_t)t->n_rel * d64;
            clr.p[1] = dE;                      clr.n[1] = (int64_t)cand->first_id * d64;
            clr.p[2] = dE + hi * d64;           clr.n[2] = ((int64_t)t->n_ent - hi) * d64;
        }
        e = launch_encode_queries(t->E, t->R, t->d, t->scorer, p, Q, g.ldq, g.Bpad, nullptr, pos->col, pos->nnz,
                                  reinterpret_cast<int32_t *>(ws + l.off_tptr), g.tiles, WIDE_TN, 0, st,
                                  (clear_grads || kl) ? &clr : nullptr);
        if (e != hipSuccess) return fail_hip(e, "encode_queries");
    }
    FusedArgs a;
    fill_wide_common(a, g, t, cand, Q);
    a.ldg = pl.ldg;
    a.pos_col = pos->col; a.pos_row = pos->row; a.nnz = pos->nnz;
    a.tile_ptr = reinterpret_cast<const int32_t *>(ws + l.off_tptr);
    a.grads_zero = (flags & OKGE_TRAIN_GRADS_ZERO) ? 1 : 0;
    a.cand_exclusive = (!cand->ids || (flags & OKGE_TRAIN_UNIQUE_CANDIDATES)) ? 1 : 0;
    a.loss_only = loss_only ? 1 : 0;
    a.G = reinterpret_cast<float *>(ws + l.off_G);
    a.dE = dE;
    a.loss_partial = reinterpret_cast<double *>(ws + l.off_loss);
    a.loss_kind = loss_kind;
    a.inv_norm = (float)(1.0 / normalizer);
    a.y_pos = 1.f; a.y_neg = 0.f;
    if (loss_kind == OKGE_LOSS_BCE && label_smoothing > 0.f) {       // trainer.py:103-105, as train_core
        const float invn = 1.0f / (float)cand->n;
        a.y_pos = (1.0f + invn) * (1.0f - label_smoothing);
        a.y_neg = (0.0f + invn) * (1.0f - label_smoothing);
    }
    auto range_of = [&](int r, int &n_lo, int &n_r, int &tiles_r) {
        n_lo = r * pl.range_n;
        n_r = std::min(pl.range_n, g.N - n_lo);
        tiles_r = (n_r + WIDE_TN - 1) / WIDE_TN;
    };
    if (scores) {
        for (int r = 0; r < pl.n_ranges; ++r) {
            int n_lo, n_r, tiles_r;
            range_of(r, n_lo, n_r, tiles_r);
            FusedArgs s = wide_range_args(a, g, n_lo, n_r);
            s.tile_ptr = nullptr; s.loss_partial = nullptr;
            s.X = scores + n_lo; s.ldx = ld_scores;
            ScopedTimer tm("wide_tile_score", st);
            e = launch_wide_tile(MODE_SCORE, s, g.row_blocks, tiles_r, st);
            if (e != hipSuccess) return fail_hip(e, "wide_tile_kernel<score>");
        }
    }
    if (kl) {
        // row log-sum-exp over ALL candidates first: (max, sum-exp) per (tile, row) of a range, merged in tile and range order
        float *row_lse = reinterpret_cast<float *>(ws + l.off_lse), *ysum = reinterpret_cast<float *>(ws + l.off_ysum);
        for (int r = 0; r < pl.n_ranges; ++r) {
            int n_lo, n_r, tiles_r;
            range_of(r, n_lo, n_r, tiles_r);
            FusedArgs s = wide_range_args(a, g, n_lo, n_r);
            s.tile_ptr = nullptr; s.loss_partial = nullptr;
            s.stats = reinterpret_cast<float *>(ws + l.off_stats);
            {
                ScopedTimer tm("wide_tile_stats", st);
                e = launch_wide_tile(MODE_STATS, s, g.row_blocks, tiles_r, st);
                if (e != hipSuccess) return fail_hip(e, "wide_tile_kernel<stats>");
            }
            ScopedTimer tm("kl_row_lse", st);
            e = launch_kl_row_lse(s.stats, tiles_r, g.B, g.Bpad, reinterpret_cast<float *>(ws + l.off_run), r == 0, r == pl.n_ranges - 1,
                                  row_lse, st, r == 0 ? pos->row : nullptr, pos->nnz, r == 0 ? ysum : nullptr);
            if (e != hipSuccess) return fail_hip(e, "kl_row_lse");
        }
        a.row_lse = row_lse;
        a.row_ysum = ysum;
    }
    const int mode = kl ? MODE_TRAIN_KL : MODE_TRAIN_BCE;
    const bool dropping = cand->drop.p > 0.f;
    const bool slice = !cand->ids && !dropping;              // the range's masked rows ARE a slice of the table
    float *Cm = reinterpret_cast<float *>(ws + l.off_Cm), *dC = reinterpret_cast<float *>(ws + l.off_dC);
    float *dQ = reinterpret_cast<float *>(ws + l.off_dQ), *slab = reinterpret_cast<float *>(ws + l.off_slab);
    for (int r = 0; r < pl.n_ranges; ++r) {
        int n_lo, n_r, tiles_r;
        range_of(r, n_lo, n_r, tiles_r);
        const FusedArgs ar = wide_range_args(a, g, n_lo, n_r);
        {
            ScopedTimer tm("wide_tile_train", st);
            e = launch_wide_tile(mode, ar, g.row_blocks, tiles_r, st);
            if (e != hipSuccess) return fail_hip(e, "wide_tile_kernel<train>");
        }
        if (loss_only) continue;
        const float *c_op = t->E + (size_t)(cand->first_id + n_lo) * t->d;
        int64_t ld_c = t->d;
        if (!slice) {
            ScopedTimer tm("wide_gather", st);
            e = launch_wide_gather(t->E, ar.cand_ids, ar.cand_first, n_lo, n_r, t->d, g.ldq, a.drop_c, a.n_table_rows, Cm, st);
            if (e != hipSuccess) return fail_hip(e, "wide_gather");
            c_op = Cm; ld_c = g.ldq;
        }
        {
            // dC = G^T . Q.  A plain slice on zero gradients: the product's rows ARE the rows of dE
            const bool direct = slice && a.grads_zero;
            {
                ScopedTimer tm("wide_dc_gemm", st);
                e = launch_gemm_f32(true, a.G, pl.ldg, Q, g.ldq, direct ? dE + (size_t)(cand->first_id + n_lo) * t->d : dC,
                                    direct ? (int64_t)t->d : (int64_t)g.ldq, n_r, t->d, g.B, 1, g.B, 0, st);
                if (e != hipSuccess) return fail_hip(e, "gemm_f32_kernel<dC>");
            }
            if (!direct) {
                ScopedTimer tm("wide_dc_scatter", st);
                e = launch_wide_dc_scatter(dC, g.ldq, ar.cand_ids, ar.cand_first, n_lo, n_r, t->d, a.drop_c, a.cand_exclusive,
                                           a.grads_zero, dE, a.n_table_rows, st);
                if (e != hipSuccess) return fail_hip(e, "wide_dc_scatter");
            }
        }
        {
            ScopedTimer tm("wide_dq_gemm", st);
            e = launch_gemm_f32(false, a.G, pl.ldg, c_op, ld_c, slab, g.ldq, g.B, t->d, n_r, pl.dq_splits, pl.dq_k_per,
                                (int64_t)g.Bpad * g.ldq, st);
            if (e != hipSuccess) return fail_hip(e, "gemm_f32_kernel<dQ>");
        }
        {
            ScopedTimer tm("wide_dq_reduce", st);
            e = launch_wide_dq_reduce(slab, pl.dq_splits, (int64_t)g.Bpad * g.ldq, g.B, t->d, g.ldq, r > 0, dQ, st);
            if (e != hipSuccess) return fail_hip(e, "wide_dq_reduce");
        }
    }
    if (loss_only) {
        ScopedTimer tm("loss_reduce", st);
        e = launch_loss_reduce(a.loss_partial, pl.n_loss_partials, loss_out, st);
        if (e != hipSuccess) return fail_hip(e, "loss_reduce");
        return OKGE_OK;
    }
    {
        ScopedTimer tm("prefix_backward", st);      // + the deterministic loss reduction
        const PrefixDev p = to_dev(*batch, t);
        e = launch_prefix_backward(t->E, t->R, t->d, t->scorer, p, dQ, 1, g.Bpad, g.ldq, nullptr, dE, dR, a.loss_partial,
                                   pl.n_loss_partials, loss_out, st, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr,
                                   (flags & OKGE_TRAIN_DISTINCT_PREFIX_ROWS) ? 1 : 0);
        if (e != hipSuccess) return fail_hip(e, "prefix_backward");
    }
    return OKGE_OK;
}

}  // namespace

int okge::report_error(int code, const std::string &msg) { return fail(code, msg); }

extern "C" {

int okge_abi_version(void) { return OKGE_ABI_VERSION; }

const char *okge_last_error(void) { return g_err.c_str(); }

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
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float *Q = reinterpret_cast<float *>(static_cast<char *>(workspace) + l.off_Q);
    const PrefixDev p = to_dev(*batch, t);
    {
        ScopedTimer tm("encode_queries", st);
        hipError_t e = launch_encode_queries(t->E, t->R, t->d, t->scorer, p, Q, g.ldq, g.Bpad, nullptr, nullptr, 0, nullptr, g.tiles, NT,
                                             0, st);
        if (e != hipSuccess) return fail_hip(e, "encode_queries");
    }
    FusedArgs a;
    fill_fused_common(a, g, t, cand, Q);     // (all rows per workgroup: rows are independent in score mode, but one pass per tile keeps C resident)
    a.X = scores;
    a.ldx = ld_scores;
    a.x_vec_ok = (ld_scores % 4 == 0) && (reinterpret_cast<uintptr_t>(scores) % 16 == 0);
    {
        ScopedTimer tm("fused_tile_score", st);
        hipError_t e = launch_sweep(g, plan_sweep(g, g.tiles, cu_count(), read_knobs()), a, st);
        if (e != hipSuccess) return fail_hip(e, "fused_tile_kernel<score>");
    }
    return OKGE_OK;
}

// Shared core of the single-device step and of the sharded okge_train_tiles.
//   q_ext   : folded queries computed elsewhere (sharded path) or nullptr (encode them here from `batch`)
//   dq_out  : if set, the dQ slabs are reduced into it and the prefix backward is left to the caller
static int train_core(const okge_tables *t, const okge_shard *sh, const okge_prefix_batch *batch, const float *q_ext,
                      int64_t ldq_ext, int32_t B, const okge_candidates *cand, const okge_positives *pos,
                      int32_t loss_kind, float label_smoothing, double normalizer, int32_t n_cand_global, int32_t flags,
                      double *loss_out, float *dE, float *dR, float *dq_out, float *scores, int64_t ld_scores,
                      const float *row_lse_ext, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!pos || pos->nnz < 0 || (pos->nnz > 0 && (!pos->col || !pos->row)))
        return fail(OKGE_ERR_INVALID, "bad positives");
    if (loss_kind != OKGE_LOSS_BCE && loss_kind != OKGE_LOSS_KL) return fail(OKGE_ERR_INVALID, "unknown loss");
    const bool loss_only = (flags & OKGE_TRAIN_LOSS_ONLY) != 0;
    if (!loss_out || (!loss_only && !dE)) return fail(OKGE_ERR_INVALID, "null output");
    if (cand->table) return fail(OKGE_ERR_INVALID, "training needs candidates from the entity table");
    if (!(normalizer > 0)) return fail(OKGE_ERR_INVALID, "normalizer must be positive");
    if (scores && ld_scores < cand->n) return fail(OKGE_ERR_INVALID, "bad scores buffer");
    Shape g;
    if (!make_shape(B, cand->n, t->d, g)) return fail(OKGE_ERR_INVALID, "bad shape");
    const SweepCtx cx = {g, cu_count(), read_knobs()};
    const TrainPlan pl = plan_train(g, cx.cus, cx.knobs);
    const TrainLayout l = train_layout(g, pl);
    if (!workspace || workspace_bytes < l.total) return fail(OKGE_ERR_WORKSPACE, "workspace too small");
    if (q_ext && ldq_ext != g.ldq) return fail(OKGE_ERR_INVALID, "query block leading dimension must be okge_query_ld(d)");
    const bool clear_grads = (flags & OKGE_TRAIN_CLEAR_GRADS) != 0 && !loss_only;
    if (clear_grads) {
        if (cand->ids || sh || !dR) return fail(OKGE_ERR_INVALID, "OKGE_TRAIN_CLEAR_GRADS needs a contiguous candidate range on an unsharded table");
        flags |= OKGE_TRAIN_GRADS_ZERO;          // the candidate rows are stored, everything else is cleared below
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace);
    const int cand_col0 = sh ? sh->cand_col0 : 0;
    hipError_t e;
    {
        // folded queries (unless supplied) + per-tile offsets into the column-sorted positives
        ScopedTimer tm("encode_queries", st);
        PrefixDev p;
        std::memset(&p, 0, sizeof(p));
        if (!q_ext) p = to_dev(*batch, t, sh);
        ClearSpec clr = {};
        // the KL loss' label mass per row is cleared HERE, by workgroups of this launch -- counted in lse_pass (own row
        // log-sum-exp) or by kl_count_pos (sharded: the log-sum-exp arrives from the exchange).  Not with hipMemsetAsync: inside a
        // captured HIP graph the memset node was not re-executed / ordered on replay (ROCm 7.2), the mass doubled every replay
        const bool kl_own_lse = loss_kind == OKGE_LOSS_KL;
        if (kl_own_lse) { clr.p[3] = reinterpret_cast<float *>(ws + l.off_ysum); clr.n[3] = g.Bpad; }
        if (clear_grads) {                        // all of dR; the rows of dE in front of and behind the candidate range
            const int64_t d64 = t->d, hi = (int64_t)cand->first_id + cand->n;
            clr.p[0] = dR;                      clr.n[0] = (int64_t)t->n_rel * d64;
            clr.p[1] = dE;                      clr.n[1] = (int64_t)cand->first_id * d64;
            clr.p[2] = dE + hi * d64;           clr.n[2] = ((int64_t)t->n_ent - hi) * d64;
        }
        // the tile kernel's gradient product reads Q as three bf16 planes: written by the launch that folds the rows, or from
        // the caller's block by a launch of its own
        v8bf *q_planes = tile_grad_split(g.KB) && !loss_only ? reinterpret_cast<v8bf *>(ws + l.off_Qp) : nullptr;
        e = launch_encode_queries(t->E, t->R, t->d, t->scorer, p, reinterpret_cast<float *>(ws + l.off_Q), g.ldq,
                                  q_ext ? 0 : g.Bpad, nullptr, pos->col, pos->nnz,
                                  reinterpret_cast<int32_t *>(ws + l.off_tptr), g.tiles, NT, cand_col0, st,
                                  (clear_grads || kl_own_lse) ? &clr : nullptr, q_planes, g.KB);
        if (e != hipSuccess) return fail_hip(e, "encode_queries");
        if (q_ext && q_planes) {
            e = launch_query_planes(q_ext, g.ldq, B, g.Bpad, g.d, g.KB, q_planes, st);
            if (e != hipSuccess) return fail_hip(e, "query_planes");
        }
    }
    FusedArgs a;
    fill_fused_common(a, g, t, cand, q_ext ? q_ext : reinterpret_cast<const float *>(ws + l.off_Q));
    a.ldg = pl.ldg;
    a.b_per_block = pl.b_per_block;
    a.cand_col0 = cand_col0;
    a.pos_col = pos->col; a.pos_row = pos->row; a.nnz = pos->nnz;
    a.tile_ptr = reinterpret_cast<const int32_t *>(ws + l.off_tptr);
    a.grads_zero = (flags & OKGE_TRAIN_GRADS_ZERO) ? 1 : 0;
    // an explicit id list may name an entity twice (precompute_batch_shared_inputs takes any list): its rows are then
    // accumulated with atomics unless the caller vouches for uniqueness (the collator's lists are unique)
    a.cand_exclusive = (!cand->ids || (flags & OKGE_TRAIN_UNIQUE_CANDIDATES)) ? 1 : 0;
    a.loss_only = loss_only ? 1 : 0;
    a.G = reinterpret_cast<float *>(ws + l.off_GT);
    if (g.KB <= 13) a.Cplanes = reinterpret_cast<v8bf *>(ws + l.off_Cm);
    else a.Cm = reinterpret_cast<float *>(ws + l.off_Cm);
    if (tile_grad_split(g.KB)) a.Qplanes = reinterpret_cast<const v8bf *>(ws + l.off_Qp);
    a.dE = dE;
    a.dC_slab = pl.dc_slabs > 0 ? reinterpret_cast<float *>(ws + l.off_dcs) : nullptr;
    a.loss_partial = reinterpret_cast<double *>(ws + l.off_loss);
    a.loss_kind = loss_kind;
    a.inv_norm = (float)(1.0 / normalizer);
    // label smoothing (trainer.py:103-105): y <- (y + 1/N) * (1 - eps), bce branch only; N = all candidates
    a.y_pos = 1.f; a.y_neg = 0.f;
    if (loss_kind == OKGE_LOSS_BCE && label_smoothing > 0.f) {
        const float invn = 1.0f / (float)(n_cand_global > 0 ? n_cand_global : cand->n);
        a.y_pos = (1.0f + invn) * (1.0f - label_smoothing);
        a.y_neg = (0.0f + invn) * (1.0f - label_smoothing);
    }
    if (scores) {
        FusedArgs s = a;
        s.X = scores; s.ldx = ld_scores;
        s.x_vec_ok = (ld_scores % 4 == 0) && (reinterpret_cast<uintptr_t>(scores) % 16 == 0);
        s.b_per_block = g.Bpad;
        ScopedTimer tm("fused_tile_score", st);
        e = launch_sweep(g, cx.plan(g.tiles), s, st);
        if (e != hipSuccess) return fail_hip(e, "fused_tile_kernel<score>");
    }
    if (loss_kind == OKGE_LOSS_KL) {
        if (sh && !row_lse_ext)
            return fail(OKGE_ERR_INVALID, "sharded KL loss: pass the all-shard row log-sum-exp (okge_row_logsumexp + exchange)");
        if (!row_lse_ext) {
            // (the label mass per row, trainer.py:99-101, is counted by extra workgroups of the pass' first kl_row_lse launch;
            //  its buffer was cleared by the encode launch above)
            if (int rc = lse_pass(cx, pl, l, a, ws, reinterpret_cast<float *>(ws + l.off_lse), st, pos->row, pos->nnz,
                                  reinterpret_cast<float *>(ws + l.off_ysum)))
                return rc;
        } else {
            ScopedTimer tm("kl_count_pos", st);   // label mass per row (trainer.py:99-101: y is not normalised)
            e = launch_kl_count_pos(pos->row, pos->nnz, g.Bpad, reinterpret_cast<float *>(ws + l.off_ysum), st);
            if (e != hipSuccess) return fail_hip(e, "kl_count_pos");
        }
        a.row_lse = row_lse_ext ? row_lse_ext : reinterpret_cast<const float *>(ws + l.off_lse);
        a.row_ysum = reinterpret_cast<const float *>(ws + l.off_ysum);
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
    const int mode = loss_kind == OKGE_LOSS_KL ? MODE_TRAIN_KL : MODE_TRAIN_BCE;
    for (int r = 0; r < pl.n_ranges; ++r) {
        int tiles_r;
        const FusedArgs ar = range_args(a, g, pl, r, tiles_r, pl.b_split);
        const int tail_r = (r == pl.n_ranges - 1 && pl.tail_split > 1) ? pl.tail_tiles : 0;     // tiles of this range launched apart
        FusedArgs at = ar;
        {
            ScopedTimer tm("fused_tile_train", st);
            if (pl.sk_wgs > 0) {                     // stream-K: a.sk_tiles tiles x sk_chunks chunks over sk_wgs workgroups
                FusedArgs as = ar;
                as.sk_tiles = tiles_r;
                e = launch_fused64(mode, as, pl.sk_wgs, 1, st);
            } else if (tail_r > 0) {
                const int main_r = tiles_r - tail_r;
                e = hipSuccess;
                if (main_r > 0) {
                    FusedArgs am = ar;
                    am.N = main_r * NT;
                    e = launch_fused64(mode, am, main_r, 1, st);
                }
                if (e == hipSuccess) {
                    at = tile_window(ar, g, main_r);
                    at.b_per_block = pl.tail_b_per_block;
                    e = launch_fused64(mode, at, tail_r, pl.tail_split, st);
                }
            } else {
                e = launch_fused64(mode, ar, tiles_r, pl.b_split, st);
            }
            if (e != hipSuccess) return fail_hip(e, "fused_tile_kernel<train>");
        }
        if (loss_only) continue;
        if (tail_r > 0) {
            ScopedTimer tm("dc_reduce", st);
            e = launch_dc_reduce(a.dC_slab, pl.dc_slabs, pl.dc_slab_rows, g.D16, at.N, g.d, at.cand_ids, at.cand_first, a.cand_exclusive,
                                 a.grads_zero, dE, a.n_table_rows, a.id_err, st);
            if (e != hipSuccess) return fail_hip(e, "dc_reduce");
        }
        if (pl.sk_wgs > 0) {
            ScopedTimer tm("dc_reduce", st);
            e = launch_dc_reduce_streamk(a.dC_slab, tiles_r, pl.sk_chunks, pl.sk_wgs, g.D16, ar.N, g.d, cand->ids, cand->first_id,
                                         a.cand_exclusive, a.grads_zero, dE, a.n_table_rows, a.id_err, st);
            if (e != hipSuccess) return fail_hip(e, "dc_reduce_streamk");
        } else if (pl.b_split > 1) {                 // (few candidate tiles: always a single range)
            ScopedTimer tm("dc_reduce", st);
            e = launch_dc_reduce(a.dC_slab, pl.dc_slabs, pl.dc_slab_rows, g.D16, g.N, g.d, cand->ids, cand->first_id, a.cand_exclusive,
                                 a.grads_zero, dE, a.n_table_rows, a.id_err, st);
            if (e != hipSuccess) return fail_hip(e, "dc_reduce");
        }
        {
            ScopedTimer tm("dq", st);
            q.N = ar.N;
            q.accumulate = r > 0 ? 1 : 0;           // later ranges add to the slabs of the first
            e = launch_dq(q, (g.Bpad / BC) * pl.nsplit, st);
            if (e != hipSuccess) return fail_hip(e, "dq_kernel");
        }
    }
    if (loss_only) {
        ScopedTimer tm("loss_reduce", st);
        e = launch_loss_reduce(a.loss_partial, pl.n_loss_partials, loss_out, st);
        if (e != hipSuccess) return fail_hip(e, "loss_reduce");
        return OKGE_OK;
    }
    if (dq_out) {
        ScopedTimer tm("slab_reduce", st);          // + the deterministic loss reduction (one extra workgroup)
        e = launch_slab_reduce(q.slab, pl.nsplit, (int64_t)g.Bpad * g.ldq, dq_out, a.loss_partial, pl.n_loss_partials,
                               loss_out, st);
        if (e != hipSuccess) return fail_hip(e, "slab_reduce");
        return OKGE_OK;
    }
    {
        ScopedTimer tm("prefix_backward", st);      // + the deterministic loss reduction (one extra workgroup)
        const PrefixDev p = to_dev(*batch, t, sh);
        e = launch_prefix_backward(t->E, t->R, t->d, t->scorer, p, q.slab, pl.nsplit, g.Bpad, g.ldq, nullptr, dE, dR,
                                   a.loss_partial, pl.n_loss_partials, loss_out, st, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr,
                                   (flags & OKGE_TRAIN_DISTINCT_PREFIX_ROWS) ? 1 : 0);
        if (e != hipSuccess) return fail_hip(e, "prefix_backward");
    }
    return OKGE_OK;
}

// ---- OKGE_TRAIN_ROW_GRADS: gradients in occurrence rows ---------------------------------------------------------------------
// The occurrence rows of the batch are gathered into two small tables behind the step's own scratch -- EV = [candidate rows |
// prefix entity rows], RV = relation rows -- and the step runs on them with positions for ids: a contiguous candidate range
// 0 .. N-1 and OKGE_TRAIN_DISTINCT_PREFIX_ROWS, the path the encoded-row ("virtual table") models take.  Every gradient row is
// then STORED once, at its position; the tile kernels are the ones every other caller runs, untouched.  Dropout counters are
// keyed by position (okge_dropout), so the masks are the dense step's.
size_t okge_train_row_grads_workspace_bytes(int32_t B, int32_t N, int32_t d)
{
    Shape s;
    if (d > 512 || !make_shape(B, N, d, s)) return 0;     // (the row-sparse step stops at slot size 512)
    return row_grads_layout(s, train_layout(s, plan_train(s, cu_count(), read_knobs())).total).total;
}

static int train_row_grads(const okge_tables *t, const okge_prefix_batch *batch, const okge_candidates *cand, const okge_positives *pos,
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
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
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
    a.vec = (t->d % 4 == 0 && (reinterpret_cast<uintptr_t>(t->E) | reinterpret_cast<uintptr_t>(t->R)) % 16 == 0) ? 1 : 0;
    {
        ScopedTimer tm("rows_gather", st);
        if (hipError_t e = launch_rows_gather(a, st); e != hipSuccess) return fail_hip(e, "rows_gather");
    }
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

int okge_train_forward_backward(const okge_tables *t, const okge_prefix_batch *batch, const okge_candidates *cand,
                                const okge_positives *pos, int32_t loss_kind, float label_smoothing,
                                double normalizer, int32_t flags, double *loss_out, float *dE, float *dR,
                                float *scores, int64_t ld_scores, void *workspace, size_t workspace_bytes,
                                void *stream)
{
    if (int rc = check_common(t, batch, cand, true)) return rc;
    if (!(flags & OKGE_TRAIN_LOSS_ONLY) && !dR) return fail(OKGE_ERR_INVALID, "null output");
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

static int check_shard(const okge_tables *t, const okge_shard *sh)
{
    if (!sh) return fail(OKGE_ERR_INVALID, "null shard descriptor");
    if (sh->ent_lo < 0 || sh->ent_hi <= sh->ent_lo || sh->ent_hi - sh->ent_lo != t->n_ent)
        return fail(OKGE_ERR_INVALID, "shard range must cover exactly the rows of the local entity table");
    return OKGE_OK;
}

int okge_encode_queries(const okge_tables *t, const okge_shard *sh, const okge_prefix_batch *batch, float *Q,
                        int64_t ldq, float *ent_rows, void *stream)
{
    okge_candidates none;
    std::memset(&none, 0, sizeof(none));
    none.n = 1; none.first_id = 0;
    if (int rc = check_common(t, batch, &none)) return rc;
    if (int rc = check_shard(t, sh)) return rc;
    if ((!Q && !ent_rows) || ldq != okge_query_ld(t->d)) return fail(OKGE_ERR_INVALID, "bad query block");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const PrefixDev p = to_dev(*batch, t, sh);
    ScopedTimer tm("encode_queries", st);
    hipError_t e = launch_encode_queries(t->E, t->R, t->d, t->scorer, p, Q, (int)ldq,
                                         okge_query_rows(batch->n_po + batch->n_sp), ent_rows, nullptr, 0, nullptr, 0,
                                         NT, 0, st);
    if (e != hipSuccess) return fail_hip(e, "encode_queries");
    return OKGE_OK;
}

int okge_fold_queries(const okge_tables *t, const okge_prefix_batch *batch, const float *ent_rows, int64_t ldq, float *Q,
                      void *stream)
{
    okge_candidates none;
    std::memset(&none, 0, sizeof(none));
    none.n = 1; none.first_id = 0;
    if (int rc = check_common(t, batch, &none)) return rc;
    if (int rc = refuse_bias(t->scorer, "okge_fold_queries", "the sharded paths are not built for it")) return rc;
    if (!ent_rows || !Q || ldq != okge_query_ld(t->d)) return fail(OKGE_ERR_INVALID, "bad query block");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    PrefixDev p = to_dev(*batch, t);
    p.ent_lo = 0; p.ent_hi = 0x7fffffff; p.whole_table = 0;     // entity ids are global here and not dereferenced: only relations are
    ScopedTimer tm("fold_queries", st);
    hipError_t e = launch_fold_queries(t->R, t->d, t->scorer, p, ent_rows, Q, (int)ldq,
                                       okge_query_rows(batch->n_po + batch->n_sp), st);
    if (e != hipSuccess) return fail_hip(e, "fold_queries");
    return OKGE_OK;
}

int okge_train_tiles(const okge_tables *t, const okge_shard *sh, const float *Q, int64_t ldq, int32_t B,
                     const okge_candidates *cand, const okge_positives *pos, int32_t loss_kind, float label_smoothing,
                     double normalizer, int32_t n_cand_global, int32_t flags, const float *row_lse, double *loss_out,
                     float *dE, float *dQ, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!t || !cand || !t->E || t->d <= 0 || t->n_ent <= 0) return fail(OKGE_ERR_INVALID, "bad tables");
    if (t->d > 512)
        return fail(OKGE_ERR_UNSUPPORTED, "slot sizes above 512 are not supported by the tile kernels: the sharded phases stop there, "
                                          "the unsharded okge_train_forward_backward takes slot sizes up to 4096");
    if (int rc = check_shard(t, sh)) return rc;
    if (!Q || !dQ || B <= 0 || cand->n <= 0) return fail(OKGE_ERR_INVALID, "bad query block / candidates");
    if (!cand->ids && (cand->first_id < 0 || (int64_t)cand->first_id + cand->n > t->n_ent))
        return fail(OKGE_ERR_INVALID, "candidate range outside the local entity table");
    return train_core(t, sh, nullptr, Q, ldq, B, cand, pos, loss_kind, label_smoothing, normalizer, n_cand_global,
                      flags, loss_out, dE, nullptr, dQ, nullptr, 0, row_lse, workspace, workspace_bytes, stream);
}

static int check_query_call(const okge_tables *t, const okge_shard *sh, const float *Q, int64_t ldq, int32_t B,
                            const okge_candidates *cand)
{
    if (!t || !cand || !t->E || t->d <= 0 || t->n_ent <= 0) return fail(OKGE_ERR_INVALID, "bad tables");
    if (t->d > 512)
        return fail(OKGE_ERR_UNSUPPORTED, "slot sizes above 512 are not supported by the tile kernels: the sharded phases stop there, "
                                          "the unsharded okge_score_prefixes / okge_train_forward_backward take slot sizes up to 4096");
    if (int rc = check_shard(t, sh)) return rc;
    if (!Q || B <= 0 || cand->n <= 0 || ldq != okge_query_ld(t->d))
        return fail(OKGE_ERR_INVALID, "bad query block / candidates");
    if (cand->table) return fail(OKGE_ERR_INVALID, "sharded calls take candidates from the local entity table");
    if (!cand->ids && (cand->first_id < 0 || (int64_t)cand->first_id + cand->n > t->n_ent))
        return fail(OKGE_ERR_INVALID, "candidate range outside the local entity table");
    return OKGE_OK;
}

int okge_score_queries(const okge_tables *t, const okge_shard *sh, const float *Q, int64_t ldq, int32_t B,
                       const okge_candidates *cand, float *scores, int64_t ld_scores, void *stream)
{
    if (int rc = check_query_call(t, sh, Q, ldq, B, cand)) return rc;
    if (!scores || ld_scores < cand->n) return fail(OKGE_ERR_INVALID, "bad scores buffer");
    Shape g;
    if (!make_shape(B, cand->n, t->d, g)) return fail(OKGE_ERR_INVALID, "bad shape");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    FusedArgs a;
    fill_fused_common(a, g, t, cand, Q);
    a.cand_col0 = sh->cand_col0;
    a.X = scores;
    a.ldx = ld_scores;
    a.x_vec_ok = (ld_scores % 4 == 0) && (reinterpret_cast<uintptr_t>(scores) % 16 == 0);
    ScopedTimer tm("fused_tile_score", st);
    hipError_t e = launch_sweep(g, plan_sweep(g, g.tiles, cu_count(), read_knobs()), a, st);
    if (e != hipSuccess) return fail_hip(e, "fused_tile_kernel<score>");
    return OKGE_OK;
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
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    FusedArgs a;
    fill_fused_common(a, g, t, cand, Q);
    a.cand_col0 = sh->cand_col0;
    return lse_pass(cx, rg, l, a, static_cast<char *>(workspace), row_lse, st);
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
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace);
    float *Q = reinterpret_cast<float *>(ws + tp.off_Q);
    const PrefixDev p = to_dev(*batch, t);
    {
        ScopedTimer tm("encode_queries", st);
        hipError_t e = launch_encode_queries(t->E, t->R, t->d, t->scorer, p, Q, g.ldq, g.Bpad, nullptr, nullptr, 0, nullptr, g.tiles, NT,
                                             0, st);
        if (e != hipSuccess) return fail_hip(e, "encode_queries");
    }
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
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    FusedArgs a;
    fill_fused_common(a, g, t, cand, Q);
    a.cand_col0 = sh->cand_col0;
    return topk_pass(cx, tp, a, static_cast<char *>(workspace), k, n_filter > 0 ? filt_ptr : nullptr, filt_col, out_scores, out_cols, nullptr, st);
}

int okge_topk_merge(const float *scores, const int32_t *cols, int32_t n_lists, int32_t B, int32_t k, float *out_scores,
                    int32_t *out_cols, void *stream)
{
    if (!scores || !cols || !out_scores || !out_cols || n_lists <= 0 || B <= 0) return fail(OKGE_ERR_INVALID, "bad lists");
    if (k < 1) return fail(OKGE_ERR_INVALID, "k must be at least 1");
    if (k > 64) return fail(OKGE_ERR_UNSUPPORTED, "top-k keeps at most 64 candidates per row");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    TopkMergeArgs m;
    std::memset(&m, 0, sizeof(m));
    m.sc = scores; m.cl = cols; m.elem_stride = 1;
    m.L = n_lists; m.rows_ld = B; m.kq = k; m.B = B; m.k = k;
    m.first = 1;
    m.out_sc = out_scores; m.out_cl = out_cols;
    ScopedTimer tm("topk_merge", st);
    hipError_t e = launch_topk_merge(m, st);
    if (e != hipSuccess) return fail_hip(e, "topk_merge");
    return OKGE_OK;
}

int okge_prefix_backward(const okge_tables *t, const okge_shard *sh, const okge_prefix_batch *batch, const float *dQ,
                         int64_t ldq, const float *ent_rows, float *dE, float *dR, void *stream)
{
    okge_candidates none;
    std::memset(&none, 0, sizeof(none));
    none.n = 1; none.first_id = 0;
    if (int rc = check_common(t, batch, &none)) return rc;
    if (int rc = check_shard(t, sh)) return rc;
    if (!dQ || !dE || !dR || ldq != okge_query_ld(t->d)) return fail(OKGE_ERR_INVALID, "bad prefix_backward arguments");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const PrefixDev p = to_dev(*batch, t, sh);
    const int B = batch->n_po + batch->n_sp;
    ScopedTimer tm("prefix_backward", st);
    hipError_t e = launch_prefix_backward(t->E, t->R, t->d, t->scorer, p, dQ, 1, okge_query_rows(B), (int)ldq, ent_rows,
                                          dE, dR, nullptr, 0, nullptr, st);
    if (e != hipSuccess) return fail_hip(e, "prefix_backward");
    return OKGE_OK;
}

int okge_prefix_backward_segmented(const okge_tables *t, const okge_shard *sh, const okge_prefix_batch *batch, const float *dQ,
                                   int64_t ldq, const float *ent_rows, const int32_t *rel_order, const int32_t *rel_seg_ptr,
                                   int32_t n_rel_seg, const int32_t *ent_order, const int32_t *ent_seg_ptr, int32_t n_ent_seg,
                                   float *grad_rows, float *dE, float *dR, void *stream)
{
    okge_candidates none;
    std::memset(&none, 0, sizeof(none));
    none.n = 1; none.first_id = 0;
    if (int rc = check_common(t, batch, &none)) return rc;
    if (int rc = check_shard(t, sh)) return rc;
    if (!dQ || !dE || !dR || ldq != okge_query_ld(t->d)) return fail(OKGE_ERR_INVALID, "bad prefix_backward arguments");
    const int B = batch->n_po + batch->n_sp;
    const bool has_r = rel_order || rel_seg_ptr || n_rel_seg, has_e = ent_order || ent_seg_ptr || n_ent_seg;
    if (!grad_rows || (!has_r && !has_e) || (has_r && (!rel_order || !rel_seg_ptr || n_rel_seg <= 0 || n_rel_seg > B)) ||
        (has_e && (!ent_order || !ent_seg_ptr || n_ent_seg <= 0 || n_ent_seg > B)))
        return fail(OKGE_ERR_INVALID, "bad row segments (order[B], seg_ptr[n_seg + 1], 1 <= n_seg <= B; grad_rows[2][rows][ldq])");
    const bool vec = t->scorer == OKGE_COMPLEX ? (t->d % 8 == 0) : (t->d % 4 == 0);
    if (!vec) return fail(OKGE_ERR_UNSUPPORTED, "segmented gradients need d % 8 == 0 (ComplEx) / d % 4 == 0 (DistMult, data-bias)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const PrefixDev p = to_dev(*batch, t, sh);
    ScopedTimer tm("prefix_backward", st);
    hipError_t e = launch_prefix_backward(t->E, t->R, t->d, t->scorer, p, dQ, 1, okge_query_rows(B), (int)ldq, ent_rows,
                                          dE, dR, nullptr, 0, nullptr, st, rel_order, rel_seg_ptr, n_rel_seg, ent_order,
                                          ent_seg_ptr, n_ent_seg, grad_rows);
    if (e != hipSuccess) return fail_hip(e, "prefix_backward_segmented");
    return OKGE_OK;
}

int okge_encode_rows(const float *table, int32_t table_rows, int32_t d, const int32_t *ids, int32_t first_id, int32_t n,
                     const okge_dropout *drop, float *out, int64_t ld_out, void *stream)
{
    if (!table || !out || d <= 0 || n < 0 || ld_out < d || table_rows <= 0)
        return fail(OKGE_ERR_INVALID, "bad encode_rows arguments");
    if (!ids && (first_id < 0 || (int64_t)first_id + n > table_rows))
        return fail(OKGE_ERR_INVALID, "row range outside the table");
    okge_dropout none;
    std::memset(&none, 0, sizeof(none));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScopedTimer tm("encode_rows", st);
    hipError_t e = launch_encode_rows(table, table_rows, d, ids, first_id, n, to_dev(drop ? *drop : none), out, ld_out, id_err_ptr(), st);
    if (e != hipSuccess) return fail_hip(e, "encode_rows");
    return OKGE_OK;
}

size_t okge_prefix_score_backward_workspace_bytes(int32_t b, int32_t n, int32_t d)
{
    return b > 0 && n > 0 && d > 0 ? score_backward_workspace_bytes(b, n, d) : 0;
}

int okge_prefix_score_backward(int32_t scorer, int32_t sp, const float *g, int64_t ld_g, int32_t b, int32_t n, const float *ent,
                               int64_t ld_ent, const float *rel, int64_t ld_rel, const float *cand, int64_t ld_cand, int32_t d,
                               float *d_ent, float *d_rel, float *d_cand, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!g || !ent || !rel || !cand || b <= 0 || n <= 0 || d <= 0 || ld_g < n || ld_ent < d || ld_rel < d || ld_cand < d)
        return fail(OKGE_ERR_INVALID, "bad prefix_score_backward arguments");
    if (!known_scorer(scorer)) return fail(OKGE_ERR_INVALID, "unknown scorer");
    if (scorer == OKGE_COMPLEX && (d & 1)) return fail(OKGE_ERR_INVALID, "ComplEx needs an even slot size");
    if (!d_ent && !d_rel && !d_cand) return OKGE_OK;
    if (!workspace || workspace_bytes < score_backward_workspace_bytes(b, n, d) || reinterpret_cast<uintptr_t>(workspace) % 16)
        return fail(OKGE_ERR_WORKSPACE, "workspace too small or unaligned (okge_prefix_score_backward_workspace_bytes)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScopedTimer tm("score_backward", st);
    hipError_t e = launch_score_backward(scorer, sp != 0, g, ld_g, b, n, ent, ld_ent, rel, ld_rel, cand, ld_cand, d, d_ent, d_rel, d_cand,
                                         workspace, st);
    if (e != hipSuccess) return fail_hip(e, "score_backward");
    return OKGE_OK;
}

int okge_scatter_rows(const float *rows, int64_t ld, const int32_t *ids, const int32_t *order, int32_t first_id, int32_t n, int32_t d,
                      const okge_dropout *drop, float *table_grad, int32_t table_rows, void *stream)
{
    if ((!rows && n > 0) || !table_grad || n < 0 || d <= 0 || ld < d || table_rows <= 0)      // (no rows: an empty tensor has no address)
        return fail(OKGE_ERR_INVALID, "bad scatter_rows arguments");
    if (!ids && (first_id < 0 || (int64_t)first_id + n > table_rows)) return fail(OKGE_ERR_INVALID, "row range outside the table");
    if (ids && n > 1 && !order) return fail(OKGE_ERR_INVALID, "scatter_rows with ids needs the positions sorted by id");
    okge_dropout none;
    std::memset(&none, 0, sizeof(none));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScopedTimer tm("scatter_rows", st);
    hipError_t e = launch_scatter_rows(rows, ld, ids, order, first_id, n, d, to_dev(drop ? *drop : none), table_grad, table_rows, id_err_ptr(), st);
    if (e != hipSuccess) return fail_hip(e, "scatter_rows");
    return OKGE_OK;
}

// ---- Tucker3 / RESCAL scorer (okge_tucker3.hip) -------------------------------------------------------------------
// workspace: [rows x d scratch of score_triples][slabs of the split products]
static size_t tucker3_scratch_bytes(int32_t B, int32_t d) { return align_up((size_t)B * d * sizeof(float), 256); }

static int check_tucker3(const float *W, int32_t d, int32_t r, int32_t B, const void *workspace, size_t workspace_bytes)
{
    if (!W || d <= 0 || r <= 0 || B <= 0) return fail(OKGE_ERR_INVALID, "bad tucker3 arguments (W, d, r_e, rows)");
    if (d > 256 || r > 256) return fail(OKGE_ERR_UNSUPPORTED, "tucker3: slot sizes / relation sizes above 256 are not supported");
    if (!workspace || workspace_bytes < okge_tucker3_workspace_bytes(B, d, r) || reinterpret_cast<uintptr_t>(workspace) % 16)
        return fail(OKGE_ERR_WORKSPACE, "workspace too small or unaligned (okge_tucker3_workspace_bytes)");
    return OKGE_OK;
}

size_t okge_tucker3_workspace_bytes(int32_t B, int32_t d, int32_t r_e)
{
    if (B <= 0 || d <= 0 || r_e <= 0 || d > 256 || r_e > 256) return 0;
    return tucker3_scratch_bytes(B, d) + tucker3_workspace_bytes(B, d, r_e, cu_count());
}

int okge_tucker3_fold(const float *W, int32_t d, int32_t r_e, const float *ent_rows, int64_t ld_ent, const float *rel_rows,
                      int64_t ld_rel, int32_t n_po, int32_t n_sp, float *Q, int64_t ldq, void *workspace, size_t workspace_bytes,
                      void *stream)
{
    if (n_po < 0 || n_sp < 0) return fail(OKGE_ERR_INVALID, "bad tucker3 arguments (row counts)");
    const int B = n_po + n_sp;
    if (int rc = check_tucker3(W, d, r_e, B, workspace, workspace_bytes)) return rc;
    if (!ent_rows || !rel_rows || !Q || ld_ent < d || ld_rel < r_e || ldq != okge_query_ld(d))
        return fail(OKGE_ERR_INVALID, "bad tucker3_fold arguments (rows, query block: ldq = okge_query_ld(d))");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float *slab = reinterpret_cast<float *>(static_cast<char *>(workspace) + tucker3_scratch_bytes(B, d));
    ScopedTimer tm("tucker3_fold", st);
    hipError_t e = launch_tucker3_fold(W, ent_rows, ld_ent, rel_rows, ld_rel, n_po, B, d, r_e, 0, Q, okge_query_rows(B), ldq, (int)ldq, slab,
                                       cu_count(), st);
    if (e != hipSuccess) return fail_hip(e, "tucker3_fold");
    return OKGE_OK;
}

int okge_tucker3_backward(const float *W, int32_t d, int32_t r_e, const float *ent_rows, int64_t ld_ent, const float *rel_rows,
                          int64_t ld_rel, const float *dQ, int64_t ldq, int32_t n_po, int32_t n_sp, int32_t flags, float *d_ent_rows,
                          float *d_rel_rows, float *dW, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n_po < 0 || n_sp < 0) return fail(OKGE_ERR_INVALID, "bad tucker3 arguments (row counts)");
    const int B = n_po + n_sp;
    if (int rc = check_tucker3(W, d, r_e, B, workspace, workspace_bytes)) return rc;
    if (!ent_rows || !rel_rows || !dQ || ld_ent < d || ld_rel < r_e || ldq < d)
        return fail(OKGE_ERR_INVALID, "bad tucker3_backward arguments (rows, dQ)");
    if (flags & ~OKGE_TRAIN_GRADS_ZERO) return fail(OKGE_ERR_INVALID, "tucker3_backward takes OKGE_TRAIN_GRADS_ZERO only");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float *slab = reinterpret_cast<float *>(static_cast<char *>(workspace) + tucker3_scratch_bytes(B, d));
    ScopedTimer tm("tucker3_backward", st);
    hipError_t e = launch_tucker3_backward(W, ent_rows, ld_ent, rel_rows, ld_rel, dQ, ldq, n_po, B, d, r_e,
                                           (flags & OKGE_TRAIN_GRADS_ZERO) ? 1 : 0, d_ent_rows, d_rel_rows, dW, slab, cu_count(), st);
    if (e != hipSuccess) return fail_hip(e, "tucker3_backward");
    return OKGE_OK;
}

int okge_tucker3_score_triples(const float *W, int32_t d, int32_t r_e, const float *subj, int64_t ld_subj, const float *rel,
                               int64_t ld_rel, const float *obj, int64_t ld_obj, int32_t n, float *out, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    if (int rc = check_tucker3(W, d, r_e, n, workspace, workspace_bytes)) return rc;
    if (!subj || !rel || !obj || !out || ld_subj < d || ld_rel < r_e || ld_obj < d)
        return fail(OKGE_ERR_INVALID, "bad tucker3_score_triples arguments");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float *q = static_cast<float *>(workspace);
    float *slab = reinterpret_cast<float *>(static_cast<char *>(workspace) + tucker3_scratch_bytes(n, d));
    ScopedTimer tm("tucker3_triples", st);
    hipError_t e = launch_tucker3_triples(W, subj, ld_subj, rel, ld_rel, obj, ld_obj, n, d, r_e, q, slab, out, cu_count(), st);
    if (e != hipSuccess) return fail_hip(e, "tucker3_score_triples");
    return OKGE_OK;
}

int okge_tucker3_apply(const float *M, int64_t ld_m, const float *x, int64_t ld_x, int32_t n, int32_t d, int32_t transpose, float *out,
                       int64_t ld_out, void *stream)
{
    if (!M || !x || !out || n < 0 || d <= 0 || ld_m < (int64_t)d * d || ld_x < d || ld_out < d)
        return fail(OKGE_ERR_INVALID, "bad tucker3_apply arguments");
    if (d > 256) return fail(OKGE_ERR_UNSUPPORTED, "tucker3: slot sizes above 256 are not supported");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScopedTimer tm("tucker3_apply", st);
    hipError_t e = launch_tucker3_apply(M, ld_m, x, ld_x, n, d, transpose != 0, out, ld_out, st);
    if (e != hipSuccess) return fail_hip(e, "tucker3_apply");
    return OKGE_OK;
}

int okge_tucker3_outer(const float *u, int64_t ld_u, const float *v, int64_t ld_v, int32_t n, int32_t d, float *out, int64_t ld_out,
                       void *stream)
{
    if (!u || !v || !out || n < 0 || d <= 0 || ld_u < d || ld_v < d || ld_out < (int64_t)d * d)
        return fail(OKGE_ERR_INVALID, "bad tucker3_outer arguments");
    if (d > 256) return fail(OKGE_ERR_UNSUPPORTED, "tucker3: slot sizes above 256 are not supported");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScopedTimer tm("tucker3_outer", st);
    hipError_t e = launch_tucker3_outer(u, ld_u, v, ld_v, n, d, out, ld_out, st);
    if (e != hipSuccess) return fail_hip(e, "tucker3_outer");
    return OKGE_OK;
}

// ---- Bigram token encoder (okge_bigram.hip) --------------------------------------------------------------------------
size_t okge_bigram_workspace_bytes(int32_t rows, int32_t max_len, int32_t d, int32_t training)
{
    return bigram_workspace_bytes(rows, max_len, d, training);
}

int okge_bigram_encode_calls(const okge_bigram_slot *s, const okge_bigram_call *calls, int32_t n_calls, int32_t training, float *out,
                             int64_t ld, int32_t *pos_tok, void *workspace, size_t workspace_bytes, void *stream)
{
    ScopedTimer tm("bigram_encode", reinterpret_cast<hipStream_t>(stream));
    return bigram_encode_calls(s, calls, n_calls, training, out, ld, pos_tok, workspace, workspace_bytes, id_err_ptr(), stream);
}

int okge_bigram_backward_calls(const okge_bigram_slot *s, const okge_bigram_call *calls, int32_t n_calls, const float *d_out,
                               int64_t ld, const int32_t *pos_tok, const int32_t *pos_order, float *dW, float *d_conv,
                               float *d_bn_weight, float *d_bn_bias, void *workspace, size_t workspace_bytes, void *stream)
{
    ScopedTimer tm("bigram_backward", reinterpret_cast<hipStream_t>(stream));
    return bigram_backward_calls(s, calls, n_calls, d_out, ld, pos_tok, pos_order, dW, d_conv, d_bn_weight, d_bn_bias, workspace,
                                 workspace_bytes, id_err_ptr(), stream);
}

// ---- LSTM token encoder (okge_lstm.hip) ----------------------------------------------------------------------------
size_t okge_lstm_workspace_bytes(int32_t rows, int32_t max_len, int32_t d, int32_t training)
{
    return lstm_workspace_bytes(rows, max_len, d, training);
}

int okge_lstm_encode_calls(const okge_lstm_slot *s, const okge_lstm_call *calls, int32_t n_calls, int32_t training, float *raw,
                           float *out, int64_t ld, int32_t *pos_tok, void *workspace, size_t workspace_bytes, void *stream)
{
    ScopedTimer tm("lstm_encode", reinterpret_cast<hipStream_t>(stream));
    return lstm_encode_calls(s, calls, n_calls, training, raw, out, ld, pos_tok, workspace, workspace_bytes, id_err_ptr(), stream);
}

int okge_lstm_backward_calls(const okge_lstm_slot *s, const okge_lstm_call *calls, int32_t n_calls, const float *raw,
                             const float *d_out, int64_t ld, const int32_t *pos_tok, const int32_t *pos_order, float *dW,
                             float *d_w_ih, float *d_w_hh, float *d_b_ih, float *d_b_hh, float *d_bn_weight, float *d_bn_bias,
                             void *workspace, size_t workspace_bytes, void *stream)
{
    ScopedTimer tm("lstm_backward", reinterpret_cast<hipStream_t>(stream));
    return lstm_backward_calls(s, calls, n_calls, raw, d_out, ld, pos_tok, pos_order, dW, d_w_ih, d_w_hh, d_b_ih, d_b_hh, d_bn_weight,
                               d_bn_bias, workspace, workspace_bytes, id_err_ptr(), stream);
}

int okge_score_triples(int32_t scorer, const float *subj, int64_t ld_subj, const float *rel, int64_t ld_rel,
                       const float *obj, int64_t ld_obj, int32_t n, int32_t d, float *out, void *stream)
{
    if (!subj || !rel || !obj || !out || n < 0 || d <= 0 || ld_subj < d || ld_rel < d || ld_obj < d)
        return fail(OKGE_ERR_INVALID, "bad score_triples arguments");
    if (!known_scorer(scorer)) return fail(OKGE_ERR_INVALID, "unknown scorer");
    if (int rc = refuse_bias(scorer, "okge_score_triples", "it scores prefixes only (model.py:311-312, :347-348)")) return rc;
    if (scorer == OKGE_COMPLEX && (d & 1)) return fail(OKGE_ERR_INVALID, "ComplEx needs an even slot size");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScopedTimer tm("score_triples", st);
    hipError_t e = launch_score_triples(subj, ld_subj, rel, ld_rel, obj, ld_obj, n, d, scorer, out, st);
    if (e != hipSuccess) return fail_hip(e, "score_triples");
    return OKGE_OK;
}

// ---- token-pooled embedder -----------------------------------------------------------------------------------------
static int check_token_embedder(const okge_token_embedder *e, const int32_t *ids, int32_t first_id, int32_t n)
{
    if (!e || !e->W || !e->token_ids || e->d <= 0 || e->vocab <= 0 || e->n_ids <= 0 || e->max_len <= 0)
        return fail(OKGE_ERR_INVALID, "bad token embedder");
    if (e->pool < 0 || e->pool > 2) return fail(OKGE_ERR_INVALID, "pool must be 0 (sum), 1 (mean) or 2 (max)");
    if (e->max_len > 64) return fail(OKGE_ERR_UNSUPPORTED, "token sequences longer than 64 are not supported");
    if (n < 0 || (!ids && (first_id < 0 || (int64_t)first_id + n > e->n_ids)))
        return fail(OKGE_ERR_INVALID, "row range outside the token-id table");
    if (e->bn_weight && (!e->bn_bias || !e->bn_running_mean || !e->bn_running_var))
        return fail(OKGE_ERR_INVALID, "batch-norm needs weight, bias and running statistics");
    return OKGE_OK;
}

size_t okge_pool_workspace_bytes(int32_t n, int32_t d) { return n > 0 && d > 0 ? pool_workspace_bytes(n, d) : 0; }

// one okge_pool_call -> the kernels' descriptor; `partial` = this call's share of the workspace
static int pool_call_dev(const okge_pool_call &c, bool backward, bool training, char *&ws, size_t &ws_left, PoolCall &q)
{
    const okge_token_embedder *e = c.e;
    if (int rc = check_token_embedder(e, c.ids, c.first_id, c.n)) return rc;
    if (c.n <= 0) return fail(OKGE_ERR_INVALID, "a pooled call needs n > 0 (leave empty calls out of the batch)");
    if (!c.raw || c.ld < e->d) return fail(OKGE_ERR_INVALID, "bad row block");
    const bool bn = e->bn_weight != nullptr;
    std::memset(&q, 0, sizeof(q));
    q.W = e->W; q.tokens = e->token_ids; q.ids = c.ids; q.raw = c.raw; q.out = c.out; q.ld = c.ld;
    q.d = e->d; q.L = e->max_len; q.first_id = c.first_id; q.n = c.n; q.pool = e->pool; q.n_ids = e->n_ids; q.vocab = e->vocab;
    q.eps = e->bn_eps; q.momentum = e->bn_momentum;
    q.bn_weight = e->bn_weight; q.bn_bias = e->bn_bias; q.run_mean = e->bn_running_mean; q.run_var = e->bn_running_var;
    if (!backward) {
        if (!c.out) return fail(OKGE_ERR_INVALID, "bad output rows");
        if (bn && c.out == c.raw)
            return fail(OKGE_ERR_INVALID, "with batch-norm the raw pooled rows are kept for backward: out must differ from raw");
        if (bn && training && !c.saved)
            return fail(OKGE_ERR_INVALID, "training-mode batch-norm needs the saved-statistics buffer (4*d floats)");
        q.saved = bn && training ? c.saved : nullptr;
    } else {
        if (!c.d_out || !c.dW) return fail(OKGE_ERR_INVALID, "bad backward arguments");
        if (bn && (!c.saved || !c.d_bn_weight || !c.d_bn_bias))
            return fail(OKGE_ERR_INVALID, "batch-norm backward needs saved statistics and gradient buffers");
        q.saved = bn ? c.saved : nullptr;
        q.dY = c.d_out; q.dW = c.dW; q.d_weight = c.d_bn_weight; q.d_bias = c.d_bn_bias;
        if (c.row_touched && (c.touched_stamp < 1 || c.touched_stamp > 255))
            return fail(OKGE_ERR_INVALID, "touched_stamp must lie in 1..255");
        q.touched = c.row_touched; q.touched_stamp = c.touched_stamp;
    }
    if (q.saved) {
        const size_t need = pool_workspace_bytes(c.n, e->d);
        if (!ws || ws_left < need) return fail(OKGE_ERR_WORKSPACE, "workspace too small (sum of okge_pool_workspace_bytes over the calls)");
        q.partial = reinterpret_cast<float *>(ws);
        ws += need;
        ws_left -= need;
    }
    return OKGE_OK;
}

int okge_pool_encode_calls(const okge_pool_call *calls, int32_t n_calls, int32_t training, void *workspace,
                           size_t workspace_bytes, void *stream)
{
    if (!calls || n_calls <= 0 || n_calls > POOL_MAX_CALLS) return fail(OKGE_ERR_INVALID, "1 to 8 pooled calls per batch");
    PoolCall q[POOL_MAX_CALLS];
    char *ws = static_cast<char *>(workspace);
    size_t left = workspace_bytes;
    for (int i = 0; i < n_calls; ++i)
        if (int rc = pool_call_dev(calls[i], false, training != 0, ws, left, q[i])) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScopedTimer tm("pool_encode", st);
    hipError_t err = launch_pool_encode_calls(q, n_calls, training != 0, id_err_ptr(), st);
    if (err != hipSuccess) return fail_hip(err, "pool_encode");
    return OKGE_OK;
}

// the calls as the kernels see them, without workspace shares (sizing only)
static int pool_calls_for_sizing(const okge_pool_call *calls, int32_t n_calls, PoolCall *q)
{
    if (!calls || n_calls <= 0 || n_calls > POOL_MAX_CALLS) return fail(OKGE_ERR_INVALID, "1 to 8 pooled calls per batch");
    for (int i = 0; i < n_calls; ++i) {
        const okge_token_embedder *e = calls[i].e;
        if (int rc = check_token_embedder(e, calls[i].ids, calls[i].first_id, calls[i].n)) return rc;
        std::memset(&q[i], 0, sizeof(PoolCall));
        q[i].tokens = e->token_ids; q[i].d = e->d; q[i].L = e->max_len; q[i].n = calls[i].n; q[i].pool = e->pool;
        q[i].vocab = e->vocab; q[i].dW = calls[i].dW; q[i].touched = calls[i].row_touched;
    }
    return OKGE_OK;
}

size_t okge_pool_scatter_state_bytes(const okge_pool_call *calls, int32_t n_calls)
{
    PoolCall q[POOL_MAX_CALLS];
    if (pool_calls_for_sizing(calls, n_calls, q)) return 0;
    return pool_scatter_state_bytes(q, n_calls);
}

size_t okge_pool_backward_workspace_bytes(const okge_pool_call *calls, int32_t n_calls)
{
    PoolCall q[POOL_MAX_CALLS];
    if (pool_calls_for_sizing(calls, n_calls, q)) return 0;
    size_t bytes = pool_scatter_workspace_bytes(q, n_calls);
    for (int i = 0; i < n_calls; ++i) bytes += pool_workspace_bytes(calls[i].n, calls[i].e->d);
    return bytes;
}

int okge_pool_backward_calls(const okge_pool_call *calls, int32_t n_calls, void *workspace, size_t workspace_bytes,
                             void *scatter_state, size_t scatter_state_bytes, void *stream)
{
    if (!calls || n_calls <= 0 || n_calls > POOL_MAX_CALLS) return fail(OKGE_ERR_INVALID, "1 to 8 pooled calls per batch");
    PoolCall q[POOL_MAX_CALLS];
    char *ws = static_cast<char *>(workspace);
    size_t left = workspace_bytes;
    for (int i = 0; i < n_calls; ++i)
        if (int rc = pool_call_dev(calls[i], true, true, ws, left, q[i])) return rc;
    if (scatter_state) {
        const size_t need_state = pool_scatter_state_bytes(q, n_calls), need_ws = pool_scatter_workspace_bytes(q, n_calls);
        if (!need_state)
            return fail(OKGE_ERR_UNSUPPORTED, "the scatter plan needs sum / mean pooling, slot sizes that are a multiple of 4 and calls "
                                              "of one token table to agree in token matrix and touched map (pass scatter_state = NULL)");
        if (scatter_state_bytes < need_state) return fail(OKGE_ERR_WORKSPACE, "scatter state too small (okge_pool_scatter_state_bytes)");
        if (!ws || left < need_ws) return fail(OKGE_ERR_WORKSPACE, "workspace too small (okge_pool_backward_workspace_bytes)");
        if (reinterpret_cast<uintptr_t>(scatter_state) % 16 || reinterpret_cast<uintptr_t>(ws) % 16)
            return fail(OKGE_ERR_INVALID, "scatter state and workspace must be 16-byte aligned");
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScopedTimer tm("pool_backward", st);
    hipError_t err = launch_pool_backward_calls(q, n_calls, id_err_ptr(), st, scatter_state, scatter_state_bytes, scatter_state ? ws : nullptr, left);
    if (err != hipSuccess) return fail_hip(err, "pool_backward");
    return OKGE_OK;
}

int okge_pool_encode(const okge_token_embedder *e, const int32_t *ids, int32_t first_id, int32_t n, int32_t training,
                     float *raw, float *out, int64_t ld, float *saved, void *workspace, size_t workspace_bytes,
                     void *stream)
{
    if (int rc = check_token_embedder(e, ids, first_id, n)) return rc;
    if (n == 0) return OKGE_OK;
    okge_pool_call c;
    std::memset(&c, 0, sizeof(c));
    c.e = e; c.ids = ids; c.first_id = first_id; c.n = n; c.raw = raw; c.out = out; c.ld = ld; c.saved = saved;
    return okge_pool_encode_calls(&c, 1, training, workspace, workspace_bytes, stream);
}

int okge_pool_backward(const okge_token_embedder *e, const int32_t *ids, int32_t first_id, int32_t n, const float *raw,
                       const float *d_out, int64_t ld, float *saved, float *dW, float *d_bn_weight, float *d_bn_bias,
                       void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = check_token_embedder(e, ids, first_id, n)) return rc;
    if (n == 0) return OKGE_OK;
    okge_pool_call c;
    std::memset(&c, 0, sizeof(c));
    c.e = e; c.ids = ids; c.first_id = first_id; c.n = n; c.raw = const_cast<float *>(raw); c.ld = ld; c.saved = saved;
    c.d_out = d_out; c.dW = dW; c.d_bn_weight = d_bn_weight; c.d_bn_bias = d_bn_bias;
    return okge_pool_backward_calls(&c, 1, workspace, workspace_bytes, nullptr, 0, stream);
}

int okge_scale_inplace(float *x, int64_t n, const float *alpha_dev, void *stream)
{
    if (!x || !alpha_dev || n < 0) return fail(OKGE_ERR_INVALID, "bad scale arguments");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScopedTimer tm("scale", st);
    hipError_t e = launch_scale(x, n, alpha_dev, st);
    if (e != hipSuccess) return fail_hip(e, "scale");
    return OKGE_OK;
}

int okge_rescale_gradients(float *g0, int64_t n0, float *g1, int64_t n1, const float *alpha_dev, float applied, void *stream)
{
    if (!g0 || !alpha_dev || n0 < 0 || n1 < 0 || (n1 > 0 && !g1) || !(applied > 0.f))
        return fail(OKGE_ERR_INVALID, "bad rescale arguments");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScopedTimer tm("rescale", st);
    hipError_t e = launch_rescale2(g0, n0, g1 ? g1 : g0, g1 ? n1 : 0, alpha_dev, applied, st);
    if (e != hipSuccess) return fail_hip(e, "rescale");
    return OKGE_OK;
}

int okge_adagrad_step(float *p, float *g, float *state_sum, int64_t n, float lr, float weight_decay, float eps,
                      int32_t zero_grad, void *stream)
{
    if (!p || !g || !state_sum || n < 0) return fail(OKGE_ERR_INVALID, "bad adagrad arguments");
    if ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(state_sum)) % 16)
        return fail(OKGE_ERR_INVALID, "adagrad buffers must be 16-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScopedTimer tm("adagrad", st);
    hipError_t e = launch_adagrad(p, g, state_sum, n, lr, weight_decay, eps, zero_grad, st);
    if (e != hipSuccess) return fail_hip(e, "adagrad");
    return OKGE_OK;
}

int okge_adagrad_step2(float *p0, float *g0, float *sum0, int64_t n0, float *p1, float *g1, float *sum1, int64_t n1,
                       float lr, float weight_decay, float eps, int32_t zero_grad, void *stream)
{
    if (!p0 || !g0 || !sum0 || n0 < 0 || !p1 || !g1 || !sum1 || n1 < 0)
        return fail(OKGE_ERR_INVALID, "bad adagrad arguments");
    if ((reinterpret_cast<uintptr_t>(p0) | reinterpret_cast<uintptr_t>(g0) | reinterpret_cast<uintptr_t>(sum0) |
         reinterpret_cast<uintptr_t>(p1) | reinterpret_cast<uintptr_t>(g1) | reinterpret_cast<uintptr_t>(sum1)) % 16)
        return fail(OKGE_ERR_INVALID, "adagrad buffers must be 16-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScopedTimer tm("adagrad", st);
    hipError_t e = launch_adagrad2(p0, g0, sum0, n0, p1, g1, sum1, n1, lr, weight_decay, eps, zero_grad, st);
    if (e != hipSuccess) return fail_hip(e, "adagrad");
    return OKGE_OK;
}

int okge_adagrad_multi(const okge_adagrad_tensor *tensors, int32_t n_tensors, float lr, float weight_decay, float eps, void *stream)
{
    if (!tensors || n_tensors <= 0 || n_tensors > ADAGRAD_MAX_SEGS) return fail(OKGE_ERR_INVALID, "1 to 4 tensors per adagrad launch");
    AdagradSegM segs[ADAGRAD_MAX_SEGS];
    for (int i = 0; i < n_tensors; ++i) {
        const okge_adagrad_tensor &t = tensors[i];
        if (!t.p || !t.g || !t.state_sum || t.n < 0) return fail(OKGE_ERR_INVALID, "bad adagrad arguments");
        if ((reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.g) | reinterpret_cast<uintptr_t>(t.state_sum)) % 16)
            return fail(OKGE_ERR_INVALID, "adagrad buffers must be 16-byte aligned");
        if (t.row_touched) {
            if (t.row_len <= 0 || t.row_len % 4 || t.n % t.row_len || t.n / t.row_len > INT32_MAX)
                return fail(OKGE_ERR_INVALID, "a touched-row map needs rows of a multiple of 4 floats that tile the tensor");
            if (t.touched_stamp < 1 || t.touched_stamp > 255) return fail(OKGE_ERR_INVALID, "touched_stamp must lie in 1..255");
            if (!t.zero_grad) return fail(OKGE_ERR_INVALID, "a touched-row map needs zero_grad (rows not stamped must hold zero gradients)");
        }
        segs[i] = AdagradSegM{t.p, t.g, t.state_sum, t.n, t.row_touched, t.row_len, t.touched_stamp, t.zero_grad};
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScopedTimer tm("adagrad", st);
    hipError_t e = launch_adagrad_multi(segs, n_tensors, lr, weight_decay, eps, st);
    if (e != hipSuccess) return fail_hip(e, "adagrad");
    return OKGE_OK;
}

// ---- okge_adagrad_rows: torch's sparse Adagrad on occurrence rows ---------------------------------------------------------------
constexpr int64_t ROWS_MAX_N = (int64_t)1 << 20;

size_t okge_adagrad_rows_workspace_bytes(int64_t n0, int64_t n1)
{
    if (n0 < 0 || n1 < 0 || n0 > ROWS_MAX_N || n1 > ROWS_MAX_N) return 0;
    Arena ar;
    if (n0 > 0) take_rows_keys(ar, n0);
    if (n1 > 0) take_rows_keys(ar, n1);
    return ar.total();
}

// one segment per tensor with n > 0, its two key buffers cut from the workspace; steps: the table's row_steps (deferred decay) or null
static void rows_segment(RowsSegs &segs, char *ws, Arena &ar, float *p, float *state_sum, const int32_t *ids, const float *g, int64_t ld_g, int32_t n,
                         int32_t table_rows, int32_t row_len, int32_t *steps)
{
    RowsSeg &sg = segs.s[segs.n_segs++];
    sg.p = p; sg.s = state_sum; sg.g = g; sg.ids = ids; sg.ld_g = ld_g;
    sg.n = n; sg.table_rows = table_rows; sg.row_len = row_len; sg.steps = steps;
    const RowsKeys keys = take_rows_keys(ar, n);
    sg.keys[0] = reinterpret_cast<uint64_t *>(ws + keys.off[0]);
    sg.keys[1] = reinterpret_cast<uint64_t *>(ws + keys.off[1]);
    sg.vec = (row_len % 4 == 0 && ld_g % 4 == 0 &&
              (reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(state_sum) | reinterpret_cast<uintptr_t>(g)) % 16 == 0) ? 1 : 0;
    // lanes per run: one per 16-byte column group up to 16 (rows of 64 floats and more: 4 runs in flight per wave, each
    // lane several independent column groups)
    const int groups = sg.vec ? row_len / 4 : row_len;
    sg.lane_shift = 0;
    while (sg.lane_shift < 4 && (1 << sg.lane_shift) < groups) ++sg.lane_shift;
}

int okge_adagrad_rows(const okge_rows_tensor *tensors, int32_t n_tensors, float lr, float eps, void *workspace, size_t workspace_bytes,
                      void *stream)
{
    if (n_tensors < 0 || n_tensors > ROWS_MAX_SEGS || (n_tensors > 0 && !tensors)) return fail(OKGE_ERR_INVALID, "one or two tensors");
    RowsSegs segs;
    std::memset(&segs, 0, sizeof(segs));
    Arena need;
    for (int k = 0; k < n_tensors; ++k) {
        const okge_rows_tensor &x = tensors[k];
        if (x.n < 0) return fail(OKGE_ERR_INVALID, "negative occurrence count");
        if (x.n > ROWS_MAX_N) return fail(OKGE_ERR_UNSUPPORTED, "okge_adagrad_rows takes up to 2^20 occurrence rows per tensor");
        if (x.n == 0) continue;
        if (!x.p || !x.state_sum || !x.ids || !x.g) return fail(OKGE_ERR_INVALID, "null tensor");
        if (x.table_rows <= 0 || x.row_len <= 0 || x.ld_g < x.row_len) return fail(OKGE_ERR_INVALID, "bad table shape / leading dimension");
        take_rows_keys(need, x.n);
    }
    if (need.total() == 0) return OKGE_OK;
    if (!workspace || workspace_bytes < need.total()) return fail(OKGE_ERR_WORKSPACE, "workspace too small (okge_adagrad_rows_workspace_bytes)");
    char *ws = static_cast<char *>(workspace);
    Arena ar;
    for (int k = 0; k < n_tensors; ++k) {
        const okge_rows_tensor &x = tensors[k];
        if (x.n > 0) rows_segment(segs, ws, ar, x.p, x.state_sum, x.ids, x.g, x.ld_g, x.n, x.table_rows, x.row_len, nullptr);
    }
    segs.id_err = id_err_ptr();
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int sorted_in = 0;
    {
        ScopedTimer tm("rows_sort", st);
        if (hipError_t e = launch_rows_sort(segs, &sorted_in, st); e != hipSuccess) return fail_hip(e, "rows_sort");
    }
    {
        ScopedTimer tm("rows_update", st);
        if (hipError_t e = launch_rows_update(segs, sorted_in, lr, eps, st); e != hipSuccess) return fail_hip(e, "rows_update");
    }
    return OKGE_OK;
}

// ---- deferred weight decay on the row-sparse step: okge_rows_catch_up, okge_adagrad_rows_decay ----------------------------------
// the table side of a tensor, which both entry points need whatever n is (lazy_rows and the sweep are float4 only)
static int rows_decay_table(const okge_rows_decay_tensor &x, const char *who)
{
    if (x.n < 0) return fail(OKGE_ERR_INVALID, "negative occurrence count");
    if (x.n > ROWS_MAX_N) return fail(OKGE_ERR_UNSUPPORTED, std::string(who) + " takes up to 2^20 occurrence rows per tensor");
    if (!x.p || !x.state_sum || !x.row_steps || x.table_rows <= 0 || x.row_len <= 0) return fail(OKGE_ERR_INVALID, "null tensor / bad table shape");
    if (x.n > 0 && !x.ids) return fail(OKGE_ERR_INVALID, "null ids");
    if (x.row_len % 4 || (reinterpret_cast<uintptr_t>(x.p) | reinterpret_cast<uintptr_t>(x.state_sum)) % 16)
        return fail(OKGE_ERR_UNSUPPORTED, "deferred weight decay needs row_len % 4 == 0 and 16-byte aligned tables");
    return OKGE_OK;
}

int okge_rows_catch_up(const okge_rows_decay_tensor *tensors, int32_t n_tensors, const int32_t *counters, float lr, float weight_decay,
                       float eps, void *stream)
{
    if (n_tensors < 0 || n_tensors > ROWS_MAX_SEGS || (n_tensors > 0 && !tensors)) return fail(OKGE_ERR_INVALID, "one or two tensors");
    if (!counters) return fail(OKGE_ERR_INVALID, "okge_rows_catch_up needs the counters");
    RowsCatchSeg segs[ROWS_MAX_SEGS];
    for (int k = 0; k < n_tensors; ++k) {
        const okge_rows_decay_tensor &x = tensors[k];
        if (int rc = rows_decay_table(x, "okge_rows_catch_up")) return rc;
        segs[k] = RowsCatchSeg{x.p, x.state_sum, x.row_steps, x.ids, x.n, x.table_rows, x.row_len, 0};
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScopedTimer tm("rows_catch_up", st);
    if (hipError_t e = launch_rows_catch_up(segs, n_tensors, counters, lr, weight_decay, eps, st); e != hipSuccess)
        return fail_hip(e, "rows_catch_up");
    return OKGE_OK;
}

int okge_adagrad_rows_decay(const okge_rows_decay_tensor *tensors, int32_t n_tensors, int32_t *counters, int32_t window, float lr,
                            float weight_decay, float eps, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n_tensors <= 0 || n_tensors > ROWS_MAX_SEGS || !tensors) return fail(OKGE_ERR_INVALID, "one or two tensors");
    if (!counters || window < 1) return fail(OKGE_ERR_INVALID, "okge_adagrad_rows_decay needs the counters and window >= 1");
    Arena need;
    for (int k = 0; k < n_tensors; ++k) {
        const okge_rows_decay_tensor &x = tensors[k];
        if (int rc = rows_decay_table(x, "okge_adagrad_rows_decay")) return rc;
        if (x.n == 0) continue;
        if (!x.g || x.ld_g < x.row_len) return fail(OKGE_ERR_INVALID, "null gradient rows / bad leading dimension");
        if (x.ld_g % 4 || reinterpret_cast<uintptr_t>(x.g) % 16)
            return fail(OKGE_ERR_UNSUPPORTED, "deferred weight decay needs ld_g % 4 == 0 and 16-byte aligned gradient rows");
        take_rows_keys(need, x.n);
    }
    if (need.total() && (!workspace || workspace_bytes < need.total())) return fail(OKGE_ERR_WORKSPACE, "workspace too small (okge_adagrad_rows_workspace_bytes)");
    RowsSegs segs;
    std::memset(&segs, 0, sizeof(segs));
    LazySeg sweep[ROWS_MAX_SEGS];
    char *ws = static_cast<char *>(workspace);
    Arena ar;
    for (int k = 0; k < n_tensors; ++k) {
        const okge_rows_decay_tensor &x = tensors[k];
        if (x.n > 0) rows_segment(segs, ws, ar, x.p, x.state_sum, x.ids, x.g, x.ld_g, x.n, x.table_rows, x.row_len, x.row_steps);
        // no row of the sweep is stamped, so its gradient operand is never read: the accumulator stands in (as in the pool catch-up)
        sweep[k] = LazySeg{x.p, x.state_sum, x.state_sum, x.row_steps, nullptr, x.table_rows, x.row_len, 0};
    }
    segs.id_err = id_err_ptr();
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (segs.n_segs) {
        int sorted_in = 0;
        {
            ScopedTimer tm("rows_sort", st);
            if (hipError_t e = launch_rows_sort(segs, &sorted_in, st); e != hipSuccess) return fail_hip(e, "rows_sort");
        }
        ScopedTimer tm("rows_update", st);
        if (hipError_t e = launch_rows_update_decay(segs, sorted_in, counters, lr, weight_decay, eps, st); e != hipSuccess)
            return fail_hip(e, "rows_update_decay");
    }
    // the due slice -- rows with r % window == T % window that the update above did not bring to T + 1 -- and T += 1 on the device
    ScopedTimer tm("rows_decay_sweep", st);
    if (hipError_t e = launch_adagrad_lazy(sweep, n_tensors, counters, window, LAZY_STEP, lr, weight_decay, eps, st); e != hipSuccess)
        return fail_hip(e, "rows_decay_sweep");
    return OKGE_OK;
}

static int lazy_tensor_dev(const okge_lazy_tensor &t, LazySeg &sg)
{
    if (!t.p || !t.g || !t.state_sum || t.rows < 0 || t.row_len <= 0) return fail(OKGE_ERR_INVALID, "bad lazy adagrad tensor");
    if (t.row_steps) {
        if (t.row_len % 4 || t.rows > INT32_MAX) return fail(OKGE_ERR_INVALID, "deferred rows need a row length that is a multiple of 4 and fewer than 2^31 rows");
        if ((reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.g) | reinterpret_cast<uintptr_t>(t.state_sum)) % 16)
            return fail(OKGE_ERR_INVALID, "adagrad buffers must be 16-byte aligned");
        if (t.row_touched && (t.touched_stamp < 1 || t.touched_stamp > 255)) return fail(OKGE_ERR_INVALID, "touched_stamp must lie in 1..255");
    } else if (t.row_touched) return fail(OKGE_ERR_INVALID, "a touched-row map needs row_steps");
    sg = LazySeg{t.p, t.g, t.state_sum, t.row_steps, t.row_touched, t.rows, t.row_len, t.touched_stamp};
    return OKGE_OK;
}

int okge_adagrad_lazy(const okge_lazy_tensor *tensors, int32_t n_tensors, int32_t *counters, int32_t window, int32_t mode, float lr,
                      float weight_decay, float eps, void *stream)
{
    if (!tensors || n_tensors <= 0 || n_tensors > ADAGRAD_MAX_SEGS) return fail(OKGE_ERR_INVALID, "1 to 4 tensors per adagrad launch");
    if (!counters || window < 1 || (mode != OKGE_LAZY_STEP && mode != OKGE_LAZY_FLUSH))
        return fail(OKGE_ERR_INVALID, "okge_adagrad_lazy needs the counters, window >= 1 and mode OKGE_LAZY_STEP / OKGE_LAZY_FLUSH");
    LazySeg segs[ADAGRAD_MAX_SEGS];
    for (int i = 0; i < n_tensors; ++i)
        if (int rc = lazy_tensor_dev(tensors[i], segs[i])) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScopedTimer tm(mode == OKGE_LAZY_STEP ? "adagrad" : "adagrad_flush", st);
    hipError_t e = launch_adagrad_lazy(segs, n_tensors, counters, window, mode, lr, weight_decay, eps, st);
    if (e != hipSuccess) return fail_hip(e, "adagrad_lazy");
    return OKGE_OK;
}

int okge_pool_catch_up_calls(const okge_pool_call *calls, int32_t n_calls, const okge_lazy_tensor *tables, int32_t n_tables,
                             const int32_t *counters, float lr, float weight_decay, float eps, void *stream)
{
    if (!calls || n_calls <= 0 || n_calls > POOL_MAX_CALLS) return fail(OKGE_ERR_INVALID, "1 to 8 pooled calls per batch");
    if (!tables || n_tables <= 0 || n_tables > ADAGRAD_MAX_SEGS || !counters) return fail(OKGE_ERR_INVALID, "bad catch-up arguments");
    PoolCall q[POOL_MAX_CALLS];
    int nq = 0;
    for (int i = 0; i < n_calls; ++i) {
        const okge_token_embedder *e = calls[i].e;
        if (int rc = check_token_embedder(e, calls[i].ids, calls[i].first_id, calls[i].n)) return rc;
        if (calls[i].n <= 0) return fail(OKGE_ERR_INVALID, "a pooled call needs n > 0 (leave empty calls out of the batch)");
        for (int j = 0; j < n_tables; ++j) {
            if (tables[j].p != e->W || !tables[j].row_steps) continue;
            LazySeg sg;
            if (int rc = lazy_tensor_dev(tables[j], sg)) return rc;
            if (tables[j].rows != e->vocab || tables[j].row_len != e->d) return fail(OKGE_ERR_INVALID, "lazy tensor and token table differ in shape");
            PoolCall &c = q[nq++];
            std::memset(&c, 0, sizeof(c));
            c.W = e->W; c.tokens = e->token_ids; c.ids = calls[i].ids; c.d = e->d; c.L = e->max_len; c.first_id = calls[i].first_id;
            c.n = calls[i].n; c.n_ids = e->n_ids; c.vocab = e->vocab; c.sumW = sg.s; c.steps = sg.steps;
            break;
        }
    }
    if (!nq) return OKGE_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScopedTimer tm("pool_catch_up", st);
    hipError_t err = launch_pool_catch_up(q, nq, counters, lr, weight_decay, eps, id_err_ptr(), st);
    if (err != hipSuccess) return fail_hip(err, "pool_catch_up");
    return OKGE_OK;
}

int okge_filtered_ranks(const float *scores, int64_t ld_scores, int32_t B, int32_t N, const int64_t *filt_ptr,
                        const int32_t *filt_col, const int64_t *row_ptr, const int64_t *grp_ptr, const int32_t *ids,
                        int64_t *ranks, void *stream)
{
    if (!scores || !filt_ptr || !row_ptr || !grp_ptr || !ids || !ranks || B <= 0 || N <= 0 || ld_scores < N)
        return fail(OKGE_ERR_INVALID, "bad rank arguments");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScopedTimer tm("filtered_ranks", st);
    hipError_t e = launch_ranks(scores, ld_scores, B, N, filt_ptr, filt_col, row_ptr, grp_ptr, ids, ranks, 0, nullptr,
                                nullptr, nullptr, st);
    if (e != hipSuccess) return fail_hip(e, "ranks");
    return OKGE_OK;
}

int okge_rank_metrics(const int64_t *ranks, int64_t n, double *acc, void *stream)
{
    if (!ranks || !acc || n < 0) return fail(OKGE_ERR_INVALID, "bad rank_metrics arguments");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScopedTimer tm("rank_metrics", st);
    hipError_t e = launch_rank_metrics(ranks, n, acc, st);
    if (e != hipSuccess) return fail_hip(e, "rank_metrics");
    return OKGE_OK;
}

// One evaluation batch on two streams: scores on `stream`, ranks + meters on `rank_stream`, ordered by events the
// library owns.  A score buffer is reused only after the ranks of the batch that last used it are counted.
}  // extern "C"
namespace {
struct EvalSlot { const float *buf; hipEvent_t scored, ranked; bool used; uint64_t last_use; };
std::mutex g_eval_mu;
std::vector<EvalSlot> g_eval_slots;
uint64_t g_eval_clock = 0;
constexpr size_t EVAL_SLOTS_MAX = 8;      // a caller alternates two (or a few) score buffers; older entries are recycled
EvalSlot &eval_slot(const float *buf)
{
    ++g_eval_clock;
    for (auto &sl : g_eval_slots)
        if (sl.buf == buf) { sl.last_use = g_eval_clock; return sl; }
    if (g_eval_slots.size() >= EVAL_SLOTS_MAX) {          // recycle the least recently used entry (its events are reused:
        size_t lru = 0;                                   // a wait on the old `ranked` event is harmless, never wrong)
        for (size_t i = 1; i < g_eval_slots.size(); ++i)
            if (g_eval_slots[i].last_use < g_eval_slots[lru].last_use) lru = i;
        g_eval_slots[lru].buf = buf;
        g_eval_slots[lru].last_use = g_eval_clock;
        return g_eval_slots[lru];
    }
    EvalSlot sl{buf, nullptr, nullptr, false, g_eval_clock};
    (void)hipEventCreateWithFlags(&sl.scored, hipEventDisableTiming);
    (void)hipEventCreateWithFlags(&sl.ranked, hipEventDisableTiming);
    g_eval_slots.push_back(sl);
    return g_eval_slots.back();
}
}  // namespace
extern "C" {

int okge_evaluate_batch(const okge_tables *t, const okge_prefix_batch *batch, const okge_candidates *cand,
                        const int64_t *filt_ptr, const int32_t *filt_col, const int64_t *row_ptr, const int64_t *grp_ptr,
                        const int32_t *ids, int64_t n_groups, float *scores, int64_t ld_scores, int64_t *ranks, double *acc,
                        void *workspace, size_t workspace_bytes, void *stream, void *rank_stream)
{
    if (!ranks || !acc || n_groups < 0) return fail(OKGE_ERR_INVALID, "bad evaluate arguments");
    hipStream_t s0 = reinterpret_cast<hipStream_t>(stream), s1 = reinterpret_cast<hipStream_t>(rank_stream);
    std::lock_guard<std::mutex> lk(g_eval_mu);
    EvalSlot &sl = eval_slot(scores);
    hipError_t e;
    if (sl.used && s0 != s1) {
        e = hipStreamWaitEvent(s0, sl.ranked, 0);
        if (e != hipSuccess) return fail_hip(e, "wait for the buffer's previous ranks");
    }
    if (int rc = okge_score_prefixes(t, batch, cand, scores, ld_scores, workspace, workspace_bytes, stream)) return rc;
    if (s0 != s1) {
        e = hipEventRecord(sl.scored, s0);
        if (e == hipSuccess) e = hipStreamWaitEvent(s1, sl.scored, 0);
        if (e != hipSuccess) return fail_hip(e, "order ranks after scores");
    }
    const int32_t B = batch->n_po + batch->n_sp;
    if (int rc = okge_filtered_ranks(scores, ld_scores, B, cand->n, filt_ptr, filt_col, row_ptr, grp_ptr, ids, ranks, rank_stream))
        return rc;
    if (int rc = okge_rank_metrics(ranks, n_groups, acc, rank_stream)) return rc;
    if (s0 != s1) {
        e = hipEventRecord(sl.ranked, s1);
        if (e != hipSuccess) return fail_hip(e, "record ranks done");
        sl.used = true;
    }
    return OKGE_OK;
}

// ---- fused evaluation: no (B, N) score block (workspace: eval_layout) -----------------------------------------------
// phases: 1 = point scores (+ queries), 2 = tile sweep, 4 = ranks + meters; okge_evaluate_fused runs all three on one
// stream, okge_evaluate_fused_phase one at a time, okge_evaluate_fused_batches pairs phase 4 of a batch with phase 1 of
// the next in one launch.
namespace {
struct EvalCall {                      // one batch's launch arguments, built once and used by whichever phases run
    Shape g;
    SweepPlan sweep_plan;
    EvalLayout eg;
    EvalPointsArgs pts;
    EvalRanksArgs rk;
    FusedArgs sweep;
    int32_t *counts;
    int64_t n_groups;
};
}  // namespace

size_t okge_eval_workspace_bytes(int32_t B, int32_t N, int32_t d, int64_t n_groups, int64_t n_filter)
{
    Shape s;
    EvalLayout e;
    return make_shape(B, N, d, s) && eval_layout(s, n_groups, n_filter, e) ? e.total : 0;
}

// Candidate-sharded call (okge_evaluate_fused_shard): folded queries from outside, the shard's candidate columns, the
// true scores in a caller-owned buffer (they are exchanged between the phases), counts instead of ranks.
struct EvalShard {
    const float *Q_in;
    int32_t      B, col_lo, n_cand_global;
    float       *true_scores;
    int64_t     *counts_out;
};

static int eval_call(EvalCall &c, const okge_tables *t, const okge_prefix_batch *batch, const okge_candidates *cand,
                     const int64_t *filt_ptr, const int32_t *filt_col, int64_t n_filter, const int64_t *row_ptr,
                     const int64_t *grp_ptr, const int32_t *ids, int64_t n_groups, int64_t *ranks, double *acc,
                     void *workspace, size_t workspace_bytes, const EvalShard *es = nullptr)
{
    if (!es) {
        if (int rc = check_common(t, batch, cand)) return rc;
    }
    if (!filt_ptr || !row_ptr || !grp_ptr || (n_groups > 0 && !ids) || (!es && (!ranks || !acc)) || n_groups < 0 || n_filter < 0 ||
        (n_filter > 0 && !filt_col))                      // (a batch without answer groups has no ids array)
        return fail(OKGE_ERR_INVALID, "bad evaluate arguments");
    if (t->d > 512)
        return fail(OKGE_ERR_UNSUPPORTED, "slot sizes above 512 are not supported by the tile kernels: fused evaluation stops there, "
                                          "okge_evaluate_batch (PipelinedEvaluator) takes slot sizes up to 4096");
    if (cand->table || cand->drop.p > 0.f || (batch && (batch->drop_po_ent.p > 0.f || batch->drop_sp_ent.p > 0.f ||
        batch->drop_po_rel.p > 0.f || batch->drop_sp_rel.p > 0.f)))
        return fail(OKGE_ERR_UNSUPPORTED, "fused evaluation is the eval-mode path (no dropout, candidates from the entity table)");
    c.n_groups = n_groups;
    if (n_groups == 0) return OKGE_OK;
    const int32_t B = es ? es->B : batch->n_po + batch->n_sp;
    Shape &g = c.g;
    EvalLayout &eg = c.eg;
    if (!make_shape(B, cand->n, t->d, g) || !eval_layout(g, n_groups, n_filter, eg)) return fail(OKGE_ERR_INVALID, "bad shape");
    c.sweep_plan = plan_sweep(g, g.tiles, cu_count(), read_knobs());
    if (!workspace || workspace_bytes < eg.total) return fail(OKGE_ERR_WORKSPACE, "workspace too small");
    char *ws = static_cast<char *>(workspace);
    float *Q = reinterpret_cast<float *>(ws + eg.off_Q), *tru = es ? es->true_scores : reinterpret_cast<float *>(ws + eg.off_true);
    float *fx = reinterpret_cast<float *>(ws + eg.off_filt);
    c.counts = reinterpret_cast<int32_t *>(ws + eg.off_counts);
    int64_t *rps = reinterpret_cast<int64_t *>(ws + eg.off_rps), *gshift = reinterpret_cast<int64_t *>(ws + eg.off_gshift);
    int32_t *grow = reinterpret_cast<int32_t *>(ws + eg.off_grow);
    EvalPointsArgs &p = c.pts;
    p.E = t->E; p.R = t->R; p.Q = Q; p.cand_ids = cand->ids;
    if (es) {                                             // rows come folded: no prefix ids here, only their number
        std::memset(&p.p, 0, sizeof(p.p));
        p.p.n_po = B;
        p.p.id_err = id_err_ptr();
    } else {
        p.p = to_dev(*batch, t);
    }
    p.Q_in = es ? es->Q_in : nullptr;
    p.col_lo = es ? es->col_lo : 0;
    p.n_cand_global = es ? es->n_cand_global : cand->n;
    p.row_ptr = row_ptr; p.grp_ptr = grp_ptr; p.filt_ptr = filt_ptr; p.ids = ids; p.filt_col = filt_col;
    p.true_out = tru; p.filt_x = fx; p.row_ptr_sorted = rps; p.gshift = gshift; p.group_row = grow;
    p.table_rows = t->n_ent; p.d = t->d; p.scorer = t->scorer; p.ldq = g.ldq; p.KB = g.KB; p.Bpad = g.Bpad;
    p.cand_first = cand->first_id; p.n_cand = cand->n;
    FusedArgs &a = c.sweep;
    fill_fused_common(a, g, t, cand, Q);
    a.rk_row_ptr = rps; a.rk_true = tru; a.rk_ngroups = n_groups;          // the sweep works on the sorted batch
    a.rk_counts = eg.slab ? nullptr : c.counts;
    a.rk_slab = eg.slab ? reinterpret_cast<uint32_t *>(c.counts) : nullptr;
    EvalRanksArgs &r = c.rk;
    r.counts = a.rk_counts; r.slab = a.rk_slab; r.true_scores = tru; r.filt_x = fx; r.filt_ptr = filt_ptr; r.gshift = gshift;
    r.group_row = grow; r.ranks = ranks; r.acc = acc; r.n_groups = n_groups; r.tiles = g.tiles; r.B = B;
    r.counts_out = es ? es->counts_out : nullptr;
    return OKGE_OK;
}

static int eval_issue(int phases, const EvalCall &c, hipStream_t st)
{
    if (c.n_groups == 0) return OKGE_OK;
    hipError_t e = hipSuccess;
    if (phases & 1) {
        if (!c.eg.slab) {
            e = hipMemsetAsync(c.counts, 0, (size_t)c.n_groups * 2 * sizeof(int32_t), st);
            if (e != hipSuccess) return fail_hip(e, "clear rank counters");
        }
        ScopedTimer tm("eval_points", st);
        e = launch_eval_side(&c.pts, nullptr, st);
        if (e != hipSuccess) return fail_hip(e, "eval_points");
    }
    if (phases & 2) {
        ScopedTimer tm("fused_tile_count", st);
        // (slot sizes above 256: the register-tile kernel's counting mode in a stream-K launch)
        e = launch_sweep(c.g, c.sweep_plan, c.sweep, st, MODE_COUNT);
        if (e != hipSuccess) return fail_hip(e, "fused_tile_kernel<count>");
    }
    if (phases & 4) {
        ScopedTimer tm("eval_ranks", st);
        e = launch_eval_side(nullptr, &c.rk, st);
        if (e != hipSuccess) return fail_hip(e, "eval_ranks");
    }
    return OKGE_OK;
}

static int evaluate_fused_impl(int phases, const okge_tables *t, const okge_prefix_batch *batch, const okge_candidates *cand,
                               const int64_t *filt_ptr, const int32_t *filt_col, int64_t n_filter, const int64_t *row_ptr,
                               const int64_t *grp_ptr, const int32_t *ids, int64_t n_groups, int64_t *ranks, double *acc,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    EvalCall c;
    if (int rc = eval_call(c, t, batch, cand, filt_ptr, filt_col, n_filter, row_ptr, grp_ptr, ids, n_groups, ranks, acc, workspace,
                           workspace_bytes))
        return rc;
    return eval_issue(phases, c, reinterpret_cast<hipStream_t>(stream));
}

int okge_evaluate_fused(const okge_tables *t, const okge_prefix_batch *batch, const okge_candidates *cand,
                        const int64_t *filt_ptr, const int32_t *filt_col, int64_t n_filter, const int64_t *row_ptr,
                        const int64_t *grp_ptr, const int32_t *ids, int64_t n_groups, int64_t *ranks, double *acc,
                        void *workspace, size_t workspace_bytes, void *stream)
{
    return evaluate_fused_impl(7, t, batch, cand, filt_ptr, filt_col, n_filter, row_ptr, grp_ptr, ids, n_groups, ranks, acc,
                               workspace, workspace_bytes, stream);
}

int okge_evaluate_fused_shard(int32_t phase, const okge_tables *t, const okge_shard *sh, const float *Q, int64_t ldq, int32_t B,
                              const okge_candidates *cand, int32_t n_cand_global, const int64_t *filt_ptr, const int32_t *filt_col,
                              int64_t n_filter, const int64_t *row_ptr, const int64_t *grp_ptr, const int32_t *ids,
                              int64_t n_groups, float *true_scores, int64_t *counts, void *workspace, size_t workspace_bytes,
                              void *stream)
{
    if (phase != 1 && phase != 2 && phase != 4) return fail(OKGE_ERR_INVALID, "phase must be 1 (points), 2 (sweep) or 4 (counts)");
    if (!t || !t->E || !t->R || t->d <= 0 || t->n_ent <= 0 || !cand || cand->n <= 0 || B <= 0 || !Q || !true_scores || !counts)
        return fail(OKGE_ERR_INVALID, "bad sharded evaluate arguments");
    if (int rc = refuse_bias(t->scorer, "okge_evaluate_fused_shard", "the sharded paths are not built for it")) return rc;
    if (int rc = check_shard(t, sh)) return rc;
    if (ldq != okge_query_ld(t->d)) return fail(OKGE_ERR_INVALID, "query block leading dimension must be okge_query_ld(d)");
    if (sh->cand_col0 < 0 || (int64_t)sh->cand_col0 + cand->n > n_cand_global)
        return fail(OKGE_ERR_INVALID, "the shard's candidate columns must lie inside the global candidate list");
    if (!cand->ids && (cand->first_id < 0 || (int64_t)cand->first_id + cand->n > t->n_ent))
        return fail(OKGE_ERR_INVALID, "candidate range outside the local entity table");
    EvalShard es;
    es.Q_in = Q; es.B = B; es.col_lo = sh->cand_col0; es.n_cand_global = n_cand_global;
    es.true_scores = true_scores; es.counts_out = counts;
    EvalCall c;
    if (int rc = eval_call(c, t, nullptr, cand, filt_ptr, filt_col, n_filter, row_ptr, grp_ptr, ids, n_groups, nullptr, nullptr,
                           workspace, workspace_bytes, &es))
        return rc;
    return eval_issue(phase, c, reinterpret_cast<hipStream_t>(stream));
}

// events of okge_evaluate_fused_batches (fork / join of the extra streams): one set per device, created on first use on that
// device.  A set is only used between the fork and the join of ONE call, and calls on one device are issued by one host
// thread at a time (the first stream orders them), so evaluators sharing a device can share the set.
constexpr int EVAL_MAX_STREAMS = 4;
static hipError_t eval_events(hipEvent_t **out)
{
    static hipEvent_t ev[OKGE_MAX_DEVICES][EVAL_MAX_STREAMS];
    static bool ready[OKGE_MAX_DEVICES] = {};
    const int dev = current_device();
    if (dev < 0) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lk(g_dev_mu);
    if (!ready[dev]) {
        for (int i = 0; i < EVAL_MAX_STREAMS; ++i) {
            hipError_t e = hipEventCreateWithFlags(&ev[dev][i], hipEventDisableTiming);
            if (e != hipSuccess) return e;
        }
        ready[dev] = true;
    }
    *out = ev[dev];
    return hipSuccess;
}

int okge_evaluate_fused_batches(const okge_tables *t, const okge_eval_batch *batches, int32_t n_batches, int64_t *ranks,
                                double *acc, void *workspace, size_t workspace_bytes, void *const *streams, int32_t n_streams)
{
    if (!batches || n_batches < 0 || !ranks || !acc || !workspace || !streams || n_streams < 1 || n_streams > EVAL_MAX_STREAMS)
        return fail(OKGE_ERR_INVALID, "bad evaluate arguments (1 to 4 streams)");
    if (n_batches == 0) return OKGE_OK;
    hipStream_t st[EVAL_MAX_STREAMS];
    for (int i = 0; i < n_streams; ++i) {
        st[i] = reinterpret_cast<hipStream_t>(streams[i]);
        for (int j = 0; j < i; ++j)
            if (st[j] == st[i]) return fail(OKGE_ERR_INVALID, "okge_evaluate_fused_batches: the streams must differ");
    }
    const int S = n_streams, slots = 2 * S;
    const size_t slot_bytes = (workspace_bytes / slots) & ~(size_t)255;
    char *ws = static_cast<char *>(workspace);
    // everything that can be refused is refused before the first launch.  Stream, workspace slot and position in the chain
    // come from the batch's index IN THE CALL -- the caller numbers its rank regions by that index too --, so a batch without
    // answer groups keeps its place and simply launches nothing (dropping it would shift the batches behind it onto other
    // chains while their rank regions stay where the caller put them: two unordered chains writing one region).
    std::vector<EvalCall> calls((size_t)n_batches);
    int live = 0;
    for (int i = 0; i < n_batches; ++i) {
        const okge_eval_batch &b = batches[i];
        if (b.rank_offset < 0) return fail(OKGE_ERR_INVALID, "negative rank_offset");
        if (int rc = eval_call(calls[i], t, &b.batch, &b.cand, b.filt_ptr, b.filt_col, b.n_filter, b.row_ptr, b.grp_ptr, b.ids,
                               b.n_groups, ranks + b.rank_offset, acc, ws + (size_t)(i % slots) * slot_bytes, slot_bytes))
            return rc;
        live += calls[i].n_groups > 0;
    }
    const int n = n_batches;
    if (live == 0) return OKGE_OK;
    // Batch i runs on stream i % S; each stream is an independent chain [points i] [sweep i] [ranks i + points i+S]
    // [sweep i+S] ... with no dependency on the others, so the device fills one chain's small latency-bound launches (and
    // the CUs a sweep's tile grid leaves empty) with the other chains' work.  2 S workspace slots: two batches in flight
    // per chain.
    hipEvent_t *ev = nullptr;
    hipError_t e = hipSuccess;
#define OKGE_EV(call, what) do { e = (call); if (e != hipSuccess) return fail_hip(e, what); } while (0)
    if (S > 1) {
        OKGE_EV(eval_events(&ev), "create evaluation events");
        OKGE_EV(hipEventRecord(ev[0], st[0]), "record fork");          // the other streams join behind whatever produced
        for (int k = 1; k < S; ++k) OKGE_EV(hipStreamWaitEvent(st[k], ev[0], 0), "fork");   // the tables / batches on the first
    }
    auto clear_counts = [&](const EvalCall &c, hipStream_t s) {      // (atomics path of very large batches only)
        return c.eg.slab ? hipSuccess : hipMemsetAsync(c.counts, 0, (size_t)c.n_groups * 2 * sizeof(int32_t), s);
    };
    for (int i = 0; i < n; ++i) {
        hipStream_t s = st[i % S];
        const bool has = calls[i].n_groups > 0;
        if (i < S && has) {                                            // head of a chain
            OKGE_EV(clear_counts(calls[i], s), "clear rank counters");
            ScopedTimer tm("eval_points", s);
            OKGE_EV(launch_eval_side(&calls[i].pts, nullptr, s), "eval_points");
        }
        if (has)
            if (int rc = eval_issue(2, calls[i], s)) return rc;
        const EvalCall *nx = (i + S < n && calls[i + S].n_groups > 0) ? &calls[i + S] : nullptr;      // the chain's next batch
        if (nx) OKGE_EV(clear_counts(*nx, s), "clear rank counters");
        if (!nx && !has) continue;
        ScopedTimer tm("eval_ranks+points", s);
        OKGE_EV(launch_eval_side(nx ? &nx->pts : nullptr, has ? &calls[i].rk : nullptr, s), "eval_side");
    }
    for (int k = 1; k < S; ++k) {
        OKGE_EV(hipEventRecord(ev[k], st[k]), "record join");
        OKGE_EV(hipStreamWaitEvent(st[0], ev[k], 0), "join");
    }
#undef OKGE_EV
    return OKGE_OK;
}

int okge_group_true_scores(const float *scores, int64_t ld_scores, int32_t B, int32_t col0, int32_t n_local,
                           const int64_t *row_ptr, const int64_t *grp_ptr, const int32_t *ids, float *true_out,
                           void *stream)
{
    if (!scores || !row_ptr || !grp_ptr || !ids || !true_out || B <= 0 || n_local <= 0 || col0 < 0 || ld_scores < n_local)
        return fail(OKGE_ERR_INVALID, "bad rank arguments");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScopedTimer tm("group_true_scores", st);
    hipError_t e = launch_ranks(scores, ld_scores, B, n_local, row_ptr /* unused */, nullptr, row_ptr, grp_ptr, ids, nullptr,
                                col0, nullptr, true_out, nullptr, st);
    if (e != hipSuccess) return fail_hip(e, "ranks<true>");
    return OKGE_OK;
}

int okge_rank_counts(const float *scores, int64_t ld_scores, int32_t B, int32_t col0, int32_t n_local,
                     const int64_t *filt_ptr, const int32_t *filt_col, const int64_t *row_ptr, const float *true_scores,
                     int64_t *counts, void *stream)
{
    if (!scores || !filt_ptr || !row_ptr || !true_scores || !counts || B <= 0 || n_local <= 0 || col0 < 0 ||
        ld_scores < n_local)
        return fail(OKGE_ERR_INVALID, "bad rank arguments");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScopedTimer tm("rank_counts", st);
    hipError_t e = launch_ranks(scores, ld_scores, B, n_local, filt_ptr, filt_col, row_ptr, nullptr, nullptr, nullptr, col0,
                                true_scores, nullptr, counts, st);
    if (e != hipSuccess) return fail_hip(e, "ranks<counts>");
    return OKGE_OK;
}

int okge_id_errors(int64_t *n_out)
{
    int *p = id_err_ptr();
    if (!p || !n_out) return fail(OKGE_ERR_INVALID, "no id error word");
    int v = 0;
    hipError_t e = hipMemcpy(&v, p, sizeof(int), hipMemcpyDeviceToHost);       // synchronises: call it when you would sync anyway
    if (e != hipSuccess) return fail_hip(e, "read id error word");
    if (v) {
        e = hipMemset(p, 0, sizeof(int));
        if (e != hipSuccess) return fail_hip(e, "clear id error word");
    }
    *n_out = v;
    return OKGE_OK;
}

int okge_clip_grad_norm(float *g0, int64_t n0, float *g1, int64_t n1, float max_norm, double *norm_out_dev, void *workspace,
                        size_t workspace_bytes, void *stream)
{
    if (!g0 || n0 < 0 || n1 < 0 || (n1 > 0 && !g1) || !(max_norm > 0.f)) return fail(OKGE_ERR_INVALID, "bad clip_grad_norm arguments");
    constexpr int NP = 1024;
    if (!workspace || workspace_bytes < NP * sizeof(double) + 256) return fail(OKGE_ERR_WORKSPACE, "workspace too small (8448 bytes)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(workspace);
    float *coef = reinterpret_cast<float *>(static_cast<char *>(workspace) + NP * sizeof(double));
    hipError_t e;
    {
        ScopedTimer tm("clip_grad_norm", st);
        e = launch_clip_coef(g0, n0, g1 ? g1 : g0, g1 ? n1 : 0, max_norm, partial, NP, coef, norm_out_dev, st);
        if (e != hipSuccess) return fail_hip(e, "clip_coef");
        e = launch_scale(g0, n0, coef, st);
        if (e == hipSuccess && g1 && n1 > 0) e = launch_scale(g1, n1, coef, st);
    }
    if (e != hipSuccess) return fail_hip(e, "scale gradients");
    return OKGE_OK;
}

int okge_merge_logsumexp(const float *parts, int32_t world, int32_t B, float *out, void *stream)
{
    if (!parts || !out || world <= 0 || B <= 0) return fail(OKGE_ERR_INVALID, "bad merge_logsumexp arguments");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScopedTimer tm("merge_lse", st);
    hipError_t e = launch_merge_lse(parts, world, B, out, st);
    if (e != hipSuccess) return fail_hip(e, "merge_lse");
    return OKGE_OK;
}

int okge_timing_enable(int32_t on)
{
    std::lock_guard<std::mutex> lk(g_tmu);
    g_timing = on != 0;
    return OKGE_OK;
}

int okge_timing_reset(void)
{
    std::lock_guard<std::mutex> lk(g_tmu);
    for (auto &t : g_launches) {
        g_event_pool.push_back(t.start);
        g_event_pool.push_back(t.stop);
    }
    g_launches.clear();
    return OKGE_OK;
}

int okge_timing_collect(const char **names, double *total_ms, int64_t *launches, int32_t cap)
{
    std::lock_guard<std::mutex> lk(g_tmu);
    int n = 0;
    for (auto &t : g_launches) {
        if (hipEventSynchronize(t.stop) != hipSuccess) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, t.start, t.stop) != hipSuccess) continue;
        int i = 0;
        for (; i < n; ++i)
            if (names[i] == t.name) break;
        if (i == n) {
            if (n >= cap) continue;
            names[n] = t.name; total_ms[n] = 0; launches[n] = 0;
            ++n;
        }
        total_ms[i] += ms;
        launches[i] += 1;
    }
    return n;
}

}  // extern "C"
