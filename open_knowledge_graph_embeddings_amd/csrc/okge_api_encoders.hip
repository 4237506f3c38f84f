// C ABI (include/okge.h), host side: the encoder models and the row utilities they run on.  Encoded rows in and out of a
// table, the score backward from a dense gradient block, triple scores, the Tucker3 / RESCAL products, the bigram and LSTM token
// encoders (bodies: okge_bigram.hip, okge_lstm.hip) and the token-pooled embedder.
#include "okge_host.h"

using namespace okge;

namespace {

const okge_dropout &or_no_dropout(const okge_dropout *drop)
{
    static const okge_dropout none = {};
    return drop ? *drop : none;
}

// ---- Tucker3 / RESCAL scorer (okge_tucker3.hip) -------------------------------------------------------------------
// workspace: [rows x d scratch of score_triples][slabs of the split products]
size_t tucker3_scratch_bytes(int32_t B, int32_t d) { return align_up((size_t)B * d * sizeof(float), 256); }
float *tucker3_slab(void *workspace, int32_t B, int32_t d) { return reinterpret_cast<float *>(static_cast<char *>(workspace) + tucker3_scratch_bytes(B, d)); }

int check_tucker3(const float *W, int32_t d, int32_t r, int32_t B, const void *workspace, size_t workspace_bytes)
{
    if (!W || d <= 0 || r <= 0 || B <= 0) return fail(OKGE_ERR_INVALID, "bad tucker3 arguments (W, d, r_e, rows)");
    if (d > 256 || r > 256) return fail(OKGE_ERR_UNSUPPORTED, "tucker3: slot sizes / relation sizes above 256 are not supported");
    if (!workspace || workspace_bytes < okge_tucker3_workspace_bytes(B, d, r) || !aligned16(workspace))
        return fail(OKGE_ERR_WORKSPACE, "workspace too small or unaligned (okge_tucker3_workspace_bytes)");
    return OKGE_OK;
}

// ---- token-pooled embedder -----------------------------------------------------------------------------------------
// one okge_pool_call -> the kernels' descriptor; `partial` = this call's share of the workspace
int pool_call_dev(const okge_pool_call &c, bool backward, bool training, char *&ws, size_t &ws_left, PoolCall &q)
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

// the calls as the kernels see them, with their shares of the workspace (ws, left: what remains of it)
int pool_calls_dev(const okge_pool_call *calls, int32_t n_calls, bool backward, bool training, char *&ws, size_t &left, PoolCall *q)
{
    if (int rc = check_pool_calls(calls, n_calls)) return rc;
    for (int i = 0; i < n_calls; ++i)
        if (int rc = pool_call_dev(calls[i], backward, training, ws, left, q[i])) return rc;
    return OKGE_OK;
}

// the calls as the kernels see them, without workspace shares (sizing only)
int pool_calls_for_sizing(const okge_pool_call *calls, int32_t n_calls, PoolCall *q)
{
    if (int rc = check_pool_calls(calls, n_calls)) return rc;
    for (int i = 0; i < n_calls; ++i) {
        const okge_token_embedder *e = calls[i].e;
        if (int rc = check_token_embedder(e, calls[i].ids, calls[i].first_id, calls[i].n)) return rc;
        std::memset(&q[i], 0, sizeof(PoolCall));
        q[i].tokens = e->token_ids; q[i].d = e->d; q[i].L = e->max_len; q[i].n = calls[i].n; q[i].pool = e->pool;
        q[i].vocab = e->vocab; q[i].dW = calls[i].dW; q[i].touched = calls[i].row_touched;
    }
    return OKGE_OK;
}

}  // namespace

int okge::check_token_embedder(const okge_token_embedder *e, const int32_t *ids, int32_t first_id, int32_t n)
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

int okge::check_pool_calls(const okge_pool_call *calls, int32_t n_calls)
{
    if (!calls || n_calls <= 0 || n_calls > POOL_MAX_CALLS) return fail(OKGE_ERR_INVALID, "1 to 8 pooled calls per batch");
    return OKGE_OK;
}

extern "C" {

int okge_encode_rows(const float *table, int32_t table_rows, int32_t d, const int32_t *ids, int32_t first_id, int32_t n,
                     const okge_dropout *drop, float *out, int64_t ld_out, void *stream)
{
    if (!table || !out || d <= 0 || n < 0 || ld_out < d || table_rows <= 0)
        return fail(OKGE_ERR_INVALID, "bad encode_rows arguments");
    if (!ids && (first_id < 0 || (int64_t)first_id + n > table_rows))
        return fail(OKGE_ERR_INVALID, "row range outside the table");
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("encode_rows", "encode_rows", st,
                      launch_encode_rows(table, table_rows, d, ids, first_id, n, to_dev(or_no_dropout(drop)), out, ld_out, id_err_ptr(), st));
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
    if (!workspace || workspace_bytes < score_backward_workspace_bytes(b, n, d) || !aligned16(workspace))
        return fail(OKGE_ERR_WORKSPACE, "workspace too small or unaligned (okge_prefix_score_backward_workspace_bytes)");
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("score_backward", "score_backward", st,
                      launch_score_backward(scorer, sp != 0, g, ld_g, b, n, ent, ld_ent, rel, ld_rel, cand, ld_cand, d, d_ent, d_rel, d_cand,
                                            workspace, st));
}

int okge_scatter_rows(const float *rows, int64_t ld, const int32_t *ids, const int32_t *order, int32_t first_id, int32_t n, int32_t d,
                      const okge_dropout *drop, float *table_grad, int32_t table_rows, void *stream)
{
    if ((!rows && n > 0) || !table_grad || n < 0 || d <= 0 || ld < d || table_rows <= 0)      // (no rows: an empty tensor has no address)
        return fail(OKGE_ERR_INVALID, "bad scatter_rows arguments");
    if (!ids && (first_id < 0 || (int64_t)first_id + n > table_rows)) return fail(OKGE_ERR_INVALID, "row range outside the table");
    if (ids && n > 1 && !order) return fail(OKGE_ERR_INVALID, "scatter_rows with ids needs the positions sorted by id");
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("scatter_rows", "scatter_rows", st,
                      launch_scatter_rows(rows, ld, ids, order, first_id, n, d, to_dev(or_no_dropout(drop)), table_grad, table_rows, id_err_ptr(),
                                          st));
}

int okge_score_triples(int32_t scorer, const float *subj, int64_t ld_subj, const float *rel, int64_t ld_rel,
                       const float *obj, int64_t ld_obj, int32_t n, int32_t d, float *out, void *stream)
{
    if (!subj || !rel || !obj || !out || n < 0 || d <= 0 || ld_subj < d || ld_rel < d || ld_obj < d)
        return fail(OKGE_ERR_INVALID, "bad score_triples arguments");
    if (!known_scorer(scorer)) return fail(OKGE_ERR_INVALID, "unknown scorer");
    if (int rc = refuse_bias(scorer, "okge_score_triples", "it scores prefixes only (model.py:311-312, :347-348)")) return rc;
    if (scorer == OKGE_COMPLEX && (d & 1)) return fail(OKGE_ERR_INVALID, "ComplEx needs an even slot size");
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("score_triples", "score_triples", st, launch_score_triples(subj, ld_subj, rel, ld_rel, obj, ld_obj, n, d, scorer, out, st));
}

// ---- Tucker3 / RESCAL scorer (okge_tucker3.hip) -------------------------------------------------------------------
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
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("tucker3_fold", "tucker3_fold", st,
                      launch_tucker3_fold(W, ent_rows, ld_ent, rel_rows, ld_rel, n_po, B, d, r_e, 0, Q, okge_query_rows(B), ldq, (int)ldq,
                                          tucker3_slab(workspace, B, d), cu_count(), st));
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
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("tucker3_backward", "tucker3_backward", st,
                      launch_tucker3_backward(W, ent_rows, ld_ent, rel_rows, ld_rel, dQ, ldq, n_po, B, d, r_e,
                                              (flags & OKGE_TRAIN_GRADS_ZERO) ? 1 : 0, d_ent_rows, d_rel_rows, dW, tucker3_slab(workspace, B, d),
                                              cu_count(), st));
}

int okge_tucker3_score_triples(const float *W, int32_t d, int32_t r_e, const float *subj, int64_t ld_subj, const float *rel,
                               int64_t ld_rel, const float *obj, int64_t ld_obj, int32_t n, float *out, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    if (int rc = check_tucker3(W, d, r_e, n, workspace, workspace_bytes)) return rc;
    if (!subj || !rel || !obj || !out || ld_subj < d || ld_rel < r_e || ld_obj < d)
        return fail(OKGE_ERR_INVALID, "bad tucker3_score_triples arguments");
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("tucker3_triples", "tucker3_score_triples", st,
                      launch_tucker3_triples(W, subj, ld_subj, rel, ld_rel, obj, ld_obj, n, d, r_e, static_cast<float *>(workspace),
                                             tucker3_slab(workspace, n, d), out, cu_count(), st));
}

int okge_tucker3_apply(const float *M, int64_t ld_m, const float *x, int64_t ld_x, int32_t n, int32_t d, int32_t transpose, float *out,
                       int64_t ld_out, void *stream)
{
    if (!M || !x || !out || n < 0 || d <= 0 || ld_m < (int64_t)d * d || ld_x < d || ld_out < d)
        return fail(OKGE_ERR_INVALID, "bad tucker3_apply arguments");
    if (d > 256) return fail(OKGE_ERR_UNSUPPORTED, "tucker3: slot sizes above 256 are not supported");
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("tucker3_apply", "tucker3_apply", st, launch_tucker3_apply(M, ld_m, x, ld_x, n, d, transpose != 0, out, ld_out, st));
}

int okge_tucker3_outer(const float *u, int64_t ld_u, const float *v, int64_t ld_v, int32_t n, int32_t d, float *out, int64_t ld_out,
                       void *stream)
{
    if (!u || !v || !out || n < 0 || d <= 0 || ld_u < d || ld_v < d || ld_out < (int64_t)d * d)
        return fail(OKGE_ERR_INVALID, "bad tucker3_outer arguments");
    if (d > 256) return fail(OKGE_ERR_UNSUPPORTED, "tucker3: slot sizes above 256 are not supported");
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("tucker3_outer", "tucker3_outer", st, launch_tucker3_outer(u, ld_u, v, ld_v, n, d, out, ld_out, st));
}

// ---- Bigram token encoder (okge_bigram.hip) --------------------------------------------------------------------------
size_t okge_bigram_workspace_bytes(int32_t rows, int32_t max_len, int32_t d, int32_t training)
{
    return bigram_workspace_bytes(rows, max_len, d, training);
}

int okge_bigram_encode_calls(const okge_bigram_slot *s, const okge_bigram_call *calls, int32_t n_calls, int32_t training, float *out,
                             int64_t ld, int32_t *pos_tok, void *workspace, size_t workspace_bytes, void *stream)
{
    ScopedTimer tm("bigram_encode", as_stream(stream));
    return bigram_encode_calls(s, calls, n_calls, training, out, ld, pos_tok, workspace, workspace_bytes, id_err_ptr(), stream);
}

int okge_bigram_backward_calls(const okge_bigram_slot *s, const okge_bigram_call *calls, int32_t n_calls, const float *d_out,
                               int64_t ld, const int32_t *pos_tok, const int32_t *pos_order, float *dW, float *d_conv,
                               float *d_bn_weight, float *d_bn_bias, void *workspace, size_t workspace_bytes, void *stream)
{
    ScopedTimer tm("bigram_backward", as_stream(stream));
    return bigram_backward_calls(s, calls, n_calls, d_out, ld, pos_tok, pos_order, dW, d_conv, d_bn_weight, d_bn_bias, workspace,
                                 workspace_bytes, id_err_ptr(), stream);
}

// ---- Lookup embedder variants (okge_lookup_encode.hip) ----------------------------------------------------------------
size_t okge_lookup_workspace_bytes(int32_t ent_rows, int32_t rel_rows, int32_t d, int32_t training)
{
    return lookup_workspace_bytes(ent_rows, rel_rows, d, training);
}

int okge_lookup_encode_calls(const okge_lookup_encoder *e, const okge_lookup_call *calls, int32_t n_calls, int32_t training,
                             float *EV, int64_t ld_e, float *RV, int64_t ld_r, void *workspace, size_t workspace_bytes,
                             void *stream)
{
    ScopedTimer tm("lookup_encode", as_stream(stream));
    return lookup_encode_calls(e, calls, n_calls, training, EV, ld_e, RV, ld_r, workspace, workspace_bytes, id_err_ptr(), stream);
}

int okge_lookup_backward_calls(const okge_lookup_encoder *e, const okge_lookup_call *calls, int32_t n_calls, const float *EV,
                               int64_t ld_e, const float *RV, int64_t ld_r, const float *dEV, int64_t ld_de, const float *dRV,
                               int64_t ld_dr, const int32_t *list_order, int32_t n_list, float *dE, float *dR,
                               float *d_bn_e_weight, float *d_bn_e_bias, float *d_bn_r_weight, float *d_bn_r_bias, float *dW_obj,
                               float *dW_subj, void *workspace, size_t workspace_bytes, void *stream)
{
    ScopedTimer tm("lookup_backward", as_stream(stream));
    return lookup_backward_calls(e, calls, n_calls, EV, ld_e, RV, ld_r, dEV, ld_de, dRV, ld_dr, list_order, n_list, dE, dR,
                                 d_bn_e_weight, d_bn_e_bias, d_bn_r_weight, d_bn_r_bias, dW_obj, dW_subj, workspace, workspace_bytes,
                                 id_err_ptr(), stream);
}

// ---- LSTM token encoder (okge_lstm.hip) ----------------------------------------------------------------------------
size_t okge_lstm_workspace_bytes(int32_t rows, int32_t max_len, int32_t d, int32_t training)
{
    return lstm_workspace_bytes(rows, max_len, d, training);
}

int okge_lstm_encode_calls(const okge_lstm_slot *s, const okge_lstm_call *calls, int32_t n_calls, int32_t training, float *raw,
                           float *out, int64_t ld, int32_t *pos_tok, void *workspace, size_t workspace_bytes, void *stream)
{
    ScopedTimer tm("lstm_encode", as_stream(stream));
    return lstm_encode_calls(s, calls, n_calls, training, raw, out, ld, pos_tok, workspace, workspace_bytes, id_err_ptr(), stream);
}

int okge_lstm_backward_calls(const okge_lstm_slot *s, const okge_lstm_call *calls, int32_t n_calls, const float *raw,
                             const float *d_out, int64_t ld, const int32_t *pos_tok, const int32_t *pos_order, float *dW,
                             float *d_w_ih, float *d_w_hh, float *d_b_ih, float *d_b_hh, float *d_bn_weight, float *d_bn_bias,
                             void *workspace, size_t workspace_bytes, void *stream)
{
    ScopedTimer tm("lstm_backward", as_stream(stream));
    return lstm_backward_calls(s, calls, n_calls, raw, d_out, ld, pos_tok, pos_order, dW, d_w_ih, d_w_hh, d_b_ih, d_b_hh, d_bn_weight,
                               d_bn_bias, workspace, workspace_bytes, id_err_ptr(), stream);
}

// ---- token-pooled embedder -----------------------------------------------------------------------------------------
size_t okge_pool_workspace_bytes(int32_t n, int32_t d) { return n > 0 && d > 0 ? pool_workspace_bytes(n, d) : 0; }

int okge_pool_encode_calls(const okge_pool_call *calls, int32_t n_calls, int32_t training, void *workspace,
                           size_t workspace_bytes, void *stream)
{
    PoolCall q[POOL_MAX_CALLS];
    char *ws = static_cast<char *>(workspace);
    size_t left = workspace_bytes;
    if (int rc = pool_calls_dev(calls, n_calls, false, training != 0, ws, left, q)) return rc;
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("pool_encode", "pool_encode", st, launch_pool_encode_calls(q, n_calls, training != 0, id_err_ptr(), st));
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
    PoolCall q[POOL_MAX_CALLS];
    char *ws = static_cast<char *>(workspace);
    size_t left = workspace_bytes;
    if (int rc = pool_calls_dev(calls, n_calls, true, true, ws, left, q)) return rc;
    if (scatter_state) {
        const size_t need_state = pool_scatter_state_bytes(q, n_calls), need_ws = pool_scatter_workspace_bytes(q, n_calls);
        if (!need_state)
            return fail(OKGE_ERR_UNSUPPORTED, "the scatter plan needs sum / mean pooling, slot sizes that are a multiple of 4 and calls "
                                              "of one token table to agree in token matrix and touched map (pass scatter_state = NULL)");
        if (scatter_state_bytes < need_state) return fail(OKGE_ERR_WORKSPACE, "scatter state too small (okge_pool_scatter_state_bytes)");
        if (!ws || left < need_ws) return fail(OKGE_ERR_WORKSPACE, "workspace too small (okge_pool_backward_workspace_bytes)");
        if (!aligned16(scatter_state, ws)) return fail(OKGE_ERR_INVALID, "scatter state and workspace must be 16-byte aligned");
    }
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("pool_backward", "pool_backward", st,
                      launch_pool_backward_calls(q, n_calls, id_err_ptr(), st, scatter_state, scatter_state_bytes, scatter_state ? ws : nullptr,
                                                 left));
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

}  // extern "C"
