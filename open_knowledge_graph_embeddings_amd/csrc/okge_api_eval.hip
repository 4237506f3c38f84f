// C ABI (include/okge.h), host side: evaluation.  Ranks and meters from a score block, the two-stream batch pipeline, fused
// evaluation (single-device, candidate-sharded, and runs of batches over several streams).
#include <vector>

#include "okge_host.h"

using namespace okge;

namespace {

// One evaluation batch on two streams (okge_evaluate_batch): scores on `stream`, ranks + meters on `rank_stream`, ordered by
// events the library owns.  A score buffer is reused only after the ranks of the batch that last used it are counted.
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

// ---- fused evaluation: no (B, N) score block (workspace: eval_layout) -----------------------------------------------
// phases: 1 = point scores (+ queries), 2 = tile sweep, 4 = ranks + meters; okge_evaluate_fused runs all three on one
// stream, okge_evaluate_fused_shard one at a time, okge_evaluate_fused_batches pairs phase 4 of a batch with phase 1 of
// the next in one launch.
struct EvalCall {                      // one batch's launch arguments, built once and used by whichever phases run
    Shape g;
    SweepPlan sweep_plan;
    EvalLayout eg;
    EvalPointsArgs pts;
    EvalRanksArgs rk;
    FusedArgs sweep;
    int32_t *counts;
    int64_t n_groups;
    // the validation loss (okge_evaluate_fused_loss / _batches_loss): a batch is then swept even without answer groups
    bool live;                         // something is launched for this batch
    int  loss_mode;                    // MODE_COUNT, or MODE_COUNT_BCE / MODE_COUNT_KL
    EvalLossPoints lpts;
    EvalLossReduce lred;
};

int check_eval_loss(const okge_eval_loss *loss)
{
    if (!loss->out) return fail(OKGE_ERR_INVALID, "okge_eval_loss: out is NULL");
    if (loss->kind != OKGE_LOSS_BCE && loss->kind != OKGE_LOSS_KL) return fail(OKGE_ERR_INVALID, "unknown loss");
    if (!(loss->label_smoothing >= 0.f && loss->label_smoothing < 1.f))
        return fail(OKGE_ERR_INVALID, "label smoothing must be in [0, 1)");
    return OKGE_OK;
}

// Candidate-sharded call (okge_evaluate_fused_shard): folded queries from outside, the shard's candidate columns, the
// true scores in a caller-owned buffer (they are exchanged between the phases), counts instead of ranks.
struct EvalShard {
    const float *Q_in;
    int32_t      B, col_lo, n_cand_global;
    float       *true_scores;
    int64_t     *counts_out;
};

int eval_call(EvalCall &c, const okge_tables *t, const okge_prefix_batch *batch, const okge_candidates *cand,
              const int64_t *filt_ptr, const int32_t *filt_col, int64_t n_filter, const int64_t *row_ptr,
              const int64_t *grp_ptr, const int32_t *ids, int64_t n_groups, int64_t *ranks, double *acc,
              void *workspace, size_t workspace_bytes, const EvalShard *es = nullptr, const okge_eval_loss *loss = nullptr,
              double *loss_out = nullptr)
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
    if (cand->table || any_dropout(batch, cand))
        return fail(OKGE_ERR_UNSUPPORTED, "fused evaluation is the eval-mode path (no dropout, candidates from the entity table)");
    c.n_groups = n_groups;
    c.live = n_groups > 0 || loss;
    c.loss_mode = !loss ? MODE_COUNT : loss->kind == OKGE_LOSS_KL ? MODE_COUNT_KL : MODE_COUNT_BCE;
    if (!c.live) return OKGE_OK;
    const int32_t B = es ? es->B : batch->n_po + batch->n_sp;
    Shape &g = c.g;
    EvalLayout &eg = c.eg;
    if (!make_shape(B, cand->n, t->d, g) || !eval_layout(g, n_groups, n_filter, eg)) return fail(OKGE_ERR_INVALID, "bad shape");
    c.sweep_plan = plan_sweep(g, g.tiles, cu_count(), read_knobs());
    const EvalLossLayout ll = eval_loss_layout(g, eg.total);
    if (!workspace || workspace_bytes < (loss ? ll.total : eg.total)) return fail(OKGE_ERR_WORKSPACE, "workspace too small");
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
    if (loss) {
        a.stats = reinterpret_cast<float *>(ws + ll.off_part);
        c.lpts.pos_sum = reinterpret_cast<double *>(ws + ll.off_pos);
        c.lpts.npos = reinterpret_cast<int32_t *>(ws + ll.off_npos);
        EvalLossReduce &q = c.lred;
        q.part = reinterpret_cast<const float2 *>(a.stats); q.pos_sum = c.lpts.pos_sum; q.npos = c.lpts.npos;
        q.rows = reinterpret_cast<double *>(ws + ll.off_rows); q.out = loss_out;
        q.smoothing = loss->kind == OKGE_LOSS_BCE ? (double)loss->label_smoothing : 0.0;
        q.tiles = g.tiles; q.B = B; q.Bpad = g.Bpad; q.N = cand->n; q.kind = loss->kind == OKGE_LOSS_KL ? LOSS_KL : LOSS_BCE;
    }
    return OKGE_OK;
}

// points of `pts` and ranks of `rk` (batches of one chain; either may be absent) in one launch, the points with the label
// term of the validation loss if their batch has one
hipError_t launch_side(const EvalCall *pts, const EvalCall *rk, hipStream_t st)
{
    if (pts && pts->loss_mode != MODE_COUNT) return launch_eval_side_loss(&pts->pts, &pts->lpts, rk ? &rk->rk : nullptr, st);
    return launch_eval_side(pts ? &pts->pts : nullptr, rk ? &rk->rk : nullptr, st);
}
// the batch's loss, after its sweep and its points
int eval_loss_issue(const EvalCall &c, hipStream_t st)
{
    if (c.loss_mode == MODE_COUNT) return OKGE_OK;
    return OKGE_TIMED("eval_loss_reduce", "eval_loss_reduce", st, launch_eval_loss_reduce(c.lred, st));
}

// the rank counters of a batch start at zero (atomics path of very large batches only: the slabs are stored whole)
int clear_counts(const EvalCall &c, hipStream_t st)
{
    if (c.eg.slab) return OKGE_OK;
    return hip_ok(hipMemsetAsync(c.counts, 0, (size_t)c.n_groups * 2 * sizeof(int32_t), st), "clear rank counters");
}

int eval_issue(int phases, const EvalCall &c, hipStream_t st)
{
    if (!c.live) return OKGE_OK;
    if (phases & 1) {
        if (int rc = clear_counts(c, st)) return rc;
        if (int rc = OKGE_TIMED("eval_points", "eval_points", st, launch_side(&c, nullptr, st))) return rc;
    }
    // (slot sizes above 256: the register-tile kernel's counting mode in a stream-K launch)
    if (phases & 2)
        if (int rc = OKGE_TIMED("fused_tile_count", "fused_tile_kernel<count>", st,
                                launch_sweep(c.g, c.sweep_plan, c.sweep, st, c.loss_mode))) return rc;
    if (phases & 4) {
        if (int rc = OKGE_TIMED("eval_ranks", "eval_ranks", st, launch_side(nullptr, &c, st))) return rc;
        if (int rc = eval_loss_issue(c, st)) return rc;
    }
    return OKGE_OK;
}

int evaluate_fused_impl(int phases, const okge_tables *t, const okge_prefix_batch *batch, const okge_candidates *cand,
                        const int64_t *filt_ptr, const int32_t *filt_col, int64_t n_filter, const int64_t *row_ptr,
                        const int64_t *grp_ptr, const int32_t *ids, int64_t n_groups, int64_t *ranks, double *acc,
                        void *workspace, size_t workspace_bytes, void *stream, const okge_eval_loss *loss = nullptr)
{
    EvalCall c;
    if (loss)
        if (int rc = check_eval_loss(loss)) return rc;
    if (int rc = eval_call(c, t, batch, cand, filt_ptr, filt_col, n_filter, row_ptr, grp_ptr, ids, n_groups, ranks, acc, workspace,
                           workspace_bytes, nullptr, loss, loss ? loss->out : nullptr))
        return rc;
    return eval_issue(phases, c, as_stream(stream));
}

// events of okge_evaluate_fused_batches (fork / join of the extra streams): one set per device, created on first use on that
// device.  A set is only used between the fork and the join of ONE call, and calls on one device are issued by one host
// thread at a time (the first stream orders them), so evaluators sharing a device can share the set.
constexpr int EVAL_MAX_STREAMS = 4;
hipError_t eval_events(hipEvent_t **out)
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

// okge_evaluate_fused_batches; loss != nullptr: okge_evaluate_fused_batches_loss (batch i's loss -> loss->out[i])
int evaluate_fused_batches_impl(const okge_tables *t, const okge_eval_batch *batches, int32_t n_batches, int64_t *ranks,
                                double *acc, void *workspace, size_t workspace_bytes, void *const *streams, int32_t n_streams,
                                const okge_eval_loss *loss)
{
    if (!batches || n_batches < 0 || !ranks || !acc || !workspace || !streams || n_streams < 1 || n_streams > EVAL_MAX_STREAMS)
        return fail(OKGE_ERR_INVALID, "bad evaluate arguments (1 to 4 streams)");
    if (n_batches == 0) return OKGE_OK;
    hipStream_t st[EVAL_MAX_STREAMS];
    for (int i = 0; i < n_streams; ++i) {
        st[i] = as_stream(streams[i]);
        for (int j = 0; j < i; ++j)
            if (st[j] == st[i]) return fail(OKGE_ERR_INVALID, "okge_evaluate_fused_batches: the streams must differ");
    }
    const int S = n_streams, slots = 2 * S;
    const size_t slot_bytes = (workspace_bytes / slots) & ~(size_t)255;
    char *ws = static_cast<char *>(workspace);
    // everything that can be refused is refused before the first launch.  Stream, workspace slot and position in the chain
    // come from the batch's index IN THE CALL -- the caller numbers its rank regions by that index too --, so a batch without
    // answer groups keeps its place and simply launches nothing (dropping it would shift the batches behind it onto other
    // chains while their rank regions stay where the caller put them: two unordered chains writing one region).  With a loss
    // every batch is live: the label-free part of its loss needs the sweep.
    std::vector<EvalCall> calls((size_t)n_batches);
    int live = 0;
    for (int i = 0; i < n_batches; ++i) {
        const okge_eval_batch &b = batches[i];
        if (b.rank_offset < 0) return fail(OKGE_ERR_INVALID, "negative rank_offset");
        if (int rc = eval_call(calls[i], t, &b.batch, &b.cand, b.filt_ptr, b.filt_col, b.n_filter, b.row_ptr, b.grp_ptr, b.ids,
                               b.n_groups, ranks + b.rank_offset, acc, ws + (size_t)(i % slots) * slot_bytes, slot_bytes, nullptr, loss,
                               loss ? loss->out + i : nullptr))
            return rc;
        live += calls[i].live;
    }
    const int n = n_batches;
    if (live == 0) return OKGE_OK;
    // Batch i runs on stream i % S; each stream is an independent chain [points i] [sweep i] [ranks i + points i+S]
    // [sweep i+S] ... with no dependency on the others, so the device fills one chain's small latency-bound launches (and
    // the CUs a sweep's tile grid leaves empty) with the other chains' work.  2 S workspace slots: two batches in flight
    // per chain.
    hipEvent_t *ev = nullptr;
    if (S > 1) {
        if (int rc = hip_ok(eval_events(&ev), "create evaluation events")) return rc;
        if (int rc = hip_ok(hipEventRecord(ev[0], st[0]), "record fork")) return rc;       // the other streams join behind whatever
        for (int k = 1; k < S; ++k)                                                        // produced the tables / batches on the first
            if (int rc = hip_ok(hipStreamWaitEvent(st[k], ev[0], 0), "fork")) return rc;
    }
    for (int i = 0; i < n; ++i) {
        hipStream_t s = st[i % S];
        const bool has = calls[i].live;
        if (i < S && has)                                              // head of a chain
            if (int rc = eval_issue(1, calls[i], s)) return rc;
        if (has)
            if (int rc = eval_issue(2, calls[i], s)) return rc;
        const EvalCall *nx = (i + S < n && calls[i + S].live) ? &calls[i + S] : nullptr;      // the chain's next batch
        if (nx)
            if (int rc = clear_counts(*nx, s)) return rc;
        if (!nx && !has) continue;
        if (int rc = OKGE_TIMED("eval_ranks+points", "eval_side", s,
                                launch_side(nx, has ? &calls[i] : nullptr, s))) return rc;
        if (has)
            if (int rc = eval_loss_issue(calls[i], s)) return rc;
    }
    for (int k = 1; k < S; ++k) {
        if (int rc = hip_ok(hipEventRecord(ev[k], st[k]), "record join")) return rc;
        if (int rc = hip_ok(hipStreamWaitEvent(st[0], ev[k], 0), "join")) return rc;
    }
    return OKGE_OK;
}

}  // namespace

extern "C" {

int okge_filtered_ranks(const float *scores, int64_t ld_scores, int32_t B, int32_t N, const int64_t *filt_ptr,
                        const int32_t *filt_col, const int64_t *row_ptr, const int64_t *grp_ptr, const int32_t *ids,
                        int64_t *ranks, void *stream)
{
    if (!scores || !filt_ptr || !row_ptr || !grp_ptr || !ids || !ranks || B <= 0 || N <= 0 || ld_scores < N)
        return fail(OKGE_ERR_INVALID, "bad rank arguments");
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("filtered_ranks", "ranks", st,
                      launch_ranks(scores, ld_scores, B, N, filt_ptr, filt_col, row_ptr, grp_ptr, ids, ranks, 0, nullptr, nullptr, nullptr, st));
}

int okge_rank_metrics(const int64_t *ranks, int64_t n, double *acc, void *stream)
{
    if (!ranks || !acc || n < 0) return fail(OKGE_ERR_INVALID, "bad rank_metrics arguments");
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("rank_metrics", "rank_metrics", st, launch_rank_metrics(ranks, n, acc, st));
}

int okge_evaluate_batch(const okge_tables *t, const okge_prefix_batch *batch, const okge_candidates *cand,
                        const int64_t *filt_ptr, const int32_t *filt_col, const int64_t *row_ptr, const int64_t *grp_ptr,
                        const int32_t *ids, int64_t n_groups, float *scores, int64_t ld_scores, int64_t *ranks, double *acc,
                        void *workspace, size_t workspace_bytes, void *stream, void *rank_stream)
{
    if (!ranks || !acc || n_groups < 0) return fail(OKGE_ERR_INVALID, "bad evaluate arguments");
    hipStream_t s0 = as_stream(stream), s1 = as_stream(rank_stream);
    std::lock_guard<std::mutex> lk(g_eval_mu);
    EvalSlot &sl = eval_slot(scores);
    if (sl.used && s0 != s1)
        if (int rc = hip_ok(hipStreamWaitEvent(s0, sl.ranked, 0), "wait for the buffer's previous ranks")) return rc;
    if (int rc = okge_score_prefixes(t, batch, cand, scores, ld_scores, workspace, workspace_bytes, stream)) return rc;
    if (s0 != s1) {
        hipError_t e = hipEventRecord(sl.scored, s0);
        if (e == hipSuccess) e = hipStreamWaitEvent(s1, sl.scored, 0);
        if (int rc = hip_ok(e, "order ranks after scores")) return rc;
    }
    const int32_t B = batch->n_po + batch->n_sp;
    if (int rc = okge_filtered_ranks(scores, ld_scores, B, cand->n, filt_ptr, filt_col, row_ptr, grp_ptr, ids, ranks, rank_stream))
        return rc;
    if (int rc = okge_rank_metrics(ranks, n_groups, acc, rank_stream)) return rc;
    if (s0 != s1) {
        if (int rc = hip_ok(hipEventRecord(sl.ranked, s1), "record ranks done")) return rc;
        sl.used = true;
    }
    return OKGE_OK;
}

size_t okge_eval_workspace_bytes(int32_t B, int32_t N, int32_t d, int64_t n_groups, int64_t n_filter)
{
    Shape s;
    EvalLayout e;
    return make_shape(B, N, d, s) && eval_layout(s, n_groups, n_filter, e) ? e.total : 0;
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
    if (int rc = check_local_range(t, cand)) return rc;
    EvalShard es;
    es.Q_in = Q; es.B = B; es.col_lo = sh->cand_col0; es.n_cand_global = n_cand_global;
    es.true_scores = true_scores; es.counts_out = counts;
    EvalCall c;
    if (int rc = eval_call(c, t, nullptr, cand, filt_ptr, filt_col, n_filter, row_ptr, grp_ptr, ids, n_groups, nullptr, nullptr,
                           workspace, workspace_bytes, &es))
        return rc;
    return eval_issue(phase, c, as_stream(stream));
}

int okge_evaluate_fused_batches(const okge_tables *t, const okge_eval_batch *batches, int32_t n_batches, int64_t *ranks,
                                double *acc, void *workspace, size_t workspace_bytes, void *const *streams, int32_t n_streams)
{
    return evaluate_fused_batches_impl(t, batches, n_batches, ranks, acc, workspace, workspace_bytes, streams, n_streams, nullptr);
}

int okge_evaluate_fused_batches_loss(const okge_tables *t, const okge_eval_batch *batches, int32_t n_batches, int64_t *ranks,
                                     double *acc, void *workspace, size_t workspace_bytes, void *const *streams, int32_t n_streams,
                                     const okge_eval_loss *loss)
{
    if (!loss) return fail(OKGE_ERR_INVALID, "okge_evaluate_fused_batches_loss: loss is NULL");
    if (int rc = check_eval_loss(loss)) return rc;
    return evaluate_fused_batches_impl(t, batches, n_batches, ranks, acc, workspace, workspace_bytes, streams, n_streams, loss);
}

size_t okge_eval_loss_workspace_bytes(int32_t B, int32_t N, int32_t d, int64_t n_groups, int64_t n_filter)
{
    Shape s;
    EvalLayout e;
    return make_shape(B, N, d, s) && eval_layout(s, n_groups, n_filter, e) ? eval_loss_layout(s, e.total).total : 0;
}

int okge_evaluate_fused_loss(const okge_tables *t, const okge_prefix_batch *batch, const okge_candidates *cand,
                             const int64_t *filt_ptr, const int32_t *filt_col, int64_t n_filter, const int64_t *row_ptr,
                             const int64_t *grp_ptr, const int32_t *ids, int64_t n_groups, int64_t *ranks, double *acc,
                             void *workspace, size_t workspace_bytes, void *stream, const okge_eval_loss *loss)
{
    if (!loss) return fail(OKGE_ERR_INVALID, "okge_evaluate_fused_loss: loss is NULL");
    return evaluate_fused_impl(7, t, batch, cand, filt_ptr, filt_col, n_filter, row_ptr, grp_ptr, ids, n_groups, ranks, acc,
                               workspace, workspace_bytes, stream, loss);
}

size_t okge_evaluate_batch_loss_workspace_bytes(int32_t B, int32_t d)
{
    const size_t base = okge_score_workspace_bytes(B, d);
    return base ? block_loss_layout(B, base).total : 0;
}

int okge_evaluate_batch_loss(const okge_tables *t, const okge_prefix_batch *batch, const okge_candidates *cand,
                             const int64_t *filt_ptr, const int32_t *filt_col, const int64_t *row_ptr, const int64_t *grp_ptr,
                             const int32_t *ids, int64_t n_groups, float *scores, int64_t ld_scores, int64_t *ranks, double *acc,
                             void *workspace, size_t workspace_bytes, void *stream, void *rank_stream, const okge_eval_loss *loss)
{
    if (!loss) return fail(OKGE_ERR_INVALID, "okge_evaluate_batch_loss: loss is NULL");
    if (int rc = check_eval_loss(loss)) return rc;
    if (!t || !batch || !cand || !row_ptr || !grp_ptr || (n_groups > 0 && !ids)) return fail(OKGE_ERR_INVALID, "bad evaluate arguments");
    const int32_t B = batch->n_po + batch->n_sp;
    const size_t base = okge_score_workspace_bytes(B, t->d);
    const BlockLossLayout l = block_loss_layout(B, base);
    if (!base || !workspace || workspace_bytes < l.total) return fail(OKGE_ERR_WORKSPACE, "workspace too small");
    // scores, ranks and meters as without a loss; then, in the rank stream's order (the score block is intact until the next
    // call that uses it, which waits for this stream), the rows' losses from the block and their sum
    hipStream_t s0 = as_stream(stream), s1 = as_stream(rank_stream);
    if (n_groups > 0) {
        if (int rc = okge_evaluate_batch(t, batch, cand, filt_ptr, filt_col, row_ptr, grp_ptr, ids, n_groups, scores, ld_scores, ranks,
                                         acc, workspace, base, stream, rank_stream))
            return rc;
    } else {
        // no answer group, nothing to rank (okge_filtered_ranks wants ids): the scores, and the loss behind them on `stream`
        if (n_groups < 0 || !scores) return fail(OKGE_ERR_INVALID, "bad evaluate arguments");
        if (s0 != s1) {
            std::lock_guard<std::mutex> lk(g_eval_mu);
            EvalSlot &sl = eval_slot(scores);
            if (sl.used)
                if (int rc = hip_ok(hipStreamWaitEvent(s0, sl.ranked, 0), "wait for the buffer's previous ranks")) return rc;
        }
        if (int rc = okge_score_prefixes(t, batch, cand, scores, ld_scores, workspace, base, stream)) return rc;
        s1 = s0;
    }
    double *rows = reinterpret_cast<double *>(static_cast<char *>(workspace) + l.off_rows);
    const int kind = loss->kind == OKGE_LOSS_KL ? LOSS_KL : LOSS_BCE;
    if (int rc = OKGE_TIMED("block_loss_rows", "block_loss_rows", s1,
                            launch_block_loss_rows(scores, ld_scores, B, cand->n, row_ptr, grp_ptr, ids, kind,
                                                   kind == LOSS_BCE ? (double)loss->label_smoothing : 0.0, rows, s1)))
        return rc;
    EvalLossReduce q;
    std::memset(&q, 0, sizeof(q));
    q.rows = rows; q.out = loss->out; q.B = B; q.N = cand->n; q.kind = kind;
    if (int rc = OKGE_TIMED("eval_loss_reduce", "eval_loss_reduce", s1, launch_eval_loss_reduce(q, s1))) return rc;
    if (s0 != s1) {                              // the buffer's next use waits for the loss as it waits for the ranks
        std::lock_guard<std::mutex> lk(g_eval_mu);
        if (int rc = hip_ok(hipEventRecord(eval_slot(scores).ranked, s1), "record loss done")) return rc;
    }
    return OKGE_OK;
}

int okge_group_true_scores(const float *scores, int64_t ld_scores, int32_t B, int32_t col0, int32_t n_local,
                           const int64_t *row_ptr, const int64_t *grp_ptr, const int32_t *ids, float *true_out,
                           void *stream)
{
    if (!scores || !row_ptr || !grp_ptr || !ids || !true_out || B <= 0 || n_local <= 0 || col0 < 0 || ld_scores < n_local)
        return fail(OKGE_ERR_INVALID, "bad rank arguments");
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("group_true_scores", "ranks<true>", st,
                      launch_ranks(scores, ld_scores, B, n_local, row_ptr /* unused */, nullptr, row_ptr, grp_ptr, ids, nullptr, col0, nullptr,
                                   true_out, nullptr, st));
}

int okge_rank_counts(const float *scores, int64_t ld_scores, int32_t B, int32_t col0, int32_t n_local,
                     const int64_t *filt_ptr, const int32_t *filt_col, const int64_t *row_ptr, const float *true_scores,
                     int64_t *counts, void *stream)
{
    if (!scores || !filt_ptr || !row_ptr || !true_scores || !counts || B <= 0 || n_local <= 0 || col0 < 0 ||
        ld_scores < n_local)
        return fail(OKGE_ERR_INVALID, "bad rank arguments");
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("rank_counts", "ranks<counts>", st,
                      launch_ranks(scores, ld_scores, B, n_local, filt_ptr, filt_col, row_ptr, nullptr, nullptr, nullptr, col0, true_scores, nullptr,
                                   counts, st));
}

}  // extern "C"
