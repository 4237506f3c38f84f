// C ABI (include/okge.h), host side: the optimizers and the gradient scaling around them.  Dense Adagrad (one, two, up to four
// tensors), the row-sparse Adagrad with and without deferred weight decay, the occurrence rows coalesced into dense gradient
// tables (okge_rows_to_dense), the lazy (deferred decay) dense step and its pool
// catch-up, dense (two or up to four tensors) and row-sparse Adam, scaling, clipping (two or up to eight tensors), and the merge of
// per-shard row log-sum-exps.
#include "okge_host.h"

using namespace okge;

namespace {

constexpr int64_t ROWS_MAX_N = (int64_t)1 << 20;       // okge_adagrad_rows: occurrence rows per tensor

int check_stamp(const void *row_touched, int32_t touched_stamp)
{
    if (row_touched && (touched_stamp < 1 || touched_stamp > 255)) return fail(OKGE_ERR_INVALID, "touched_stamp must lie in 1..255");
    return OKGE_OK;
}

// the touched-row map of a dense tensor of n floats (okge_adagrad_multi, okge_adam_multi, okge_clip_grad_norm_multi)
int check_touched_rows(const void *row_touched, int32_t row_len, int32_t touched_stamp, int64_t n)
{
    if (!row_touched) return OKGE_OK;
    if (row_len <= 0 || row_len % 4 || n % row_len || n / row_len > INT32_MAX)
        return fail(OKGE_ERR_INVALID, "a touched-row map needs rows of a multiple of 4 floats that tile the tensor");
    return check_stamp(row_touched, touched_stamp);
}

int check_adagrad(const float *p, const float *g, const float *state_sum, int64_t n)
{
    if (!p || !g || !state_sum || n < 0) return fail(OKGE_ERR_INVALID, "bad adagrad arguments");
    if (!aligned16(p, g, state_sum)) return fail(OKGE_ERR_INVALID, "adagrad buffers must be 16-byte aligned");
    return OKGE_OK;
}

int check_rows_count(const void *tensors, int32_t n_tensors, int32_t at_least)
{
    if (n_tensors < at_least || n_tensors > ROWS_MAX_SEGS || (n_tensors > 0 && !tensors)) return fail(OKGE_ERR_INVALID, "one or two tensors");
    return OKGE_OK;
}

// one segment per tensor with n > 0, its two key buffers cut from the workspace; steps: the table's row_steps (deferred decay) or null
void rows_segment(RowsSegs &segs, char *ws, Arena &ar, float *p, float *state_sum, const int32_t *ids, const float *g, int64_t ld_g, int32_t n,
                  int32_t table_rows, int32_t row_len, int32_t *steps, float *second_moment = nullptr, const int32_t *adam_state = nullptr)
{
    RowsSeg &sg = segs.s[segs.n_segs++];
    sg.p = p; sg.s = state_sum; sg.g = g; sg.ids = ids; sg.ld_g = ld_g;
    sg.n = n; sg.table_rows = table_rows; sg.row_len = row_len; sg.steps = steps;
    sg.s2 = second_moment; sg.state = adam_state;                  // (okge_adam_rows: state_sum is exp_avg)
    const RowsKeys keys = take_rows_keys(ar, n);
    sg.keys[0] = reinterpret_cast<uint64_t *>(ws + keys.off[0]);
    sg.keys[1] = reinterpret_cast<uint64_t *>(ws + keys.off[1]);
    sg.vec = (row_len % 4 == 0 && ld_g % 4 == 0 && aligned16(p, state_sum, g, second_moment)) ? 1 : 0;
    // lanes per run: one per 16-byte column group up to 16 (rows of 64 floats and more: 4 runs in flight per wave, each
    // lane several independent column groups)
    const int groups = sg.vec ? row_len / 4 : row_len;
    sg.lane_shift = 0;
    while (sg.lane_shift < 4 && (1 << sg.lane_shift) < groups) ++sg.lane_shift;
}

int rows_sort(const RowsSegs &segs, int *sorted_in, hipStream_t st)
{
    return OKGE_TIMED("rows_sort", "rows_sort", st, launch_rows_sort(segs, sorted_in, st));
}

// ---- deferred weight decay on the row-sparse step: okge_rows_catch_up, okge_adagrad_rows_decay ----------------------------------
// the table side of a tensor, which both entry points need whatever n is (lazy_rows and the sweep are float4 only)
int rows_decay_table(const okge_rows_decay_tensor &x, const char *who)
{
    if (x.n < 0) return fail(OKGE_ERR_INVALID, "negative occurrence count");
    if (x.n > ROWS_MAX_N) return fail(OKGE_ERR_UNSUPPORTED, std::string(who) + " takes up to 2^20 occurrence rows per tensor");
    if (!x.p || !x.state_sum || !x.row_steps || x.table_rows <= 0 || x.row_len <= 0) return fail(OKGE_ERR_INVALID, "null tensor / bad table shape");
    if (x.n > 0 && !x.ids) return fail(OKGE_ERR_INVALID, "null ids");
    if (x.row_len % 4 || !aligned16(x.p, x.state_sum))
        return fail(OKGE_ERR_UNSUPPORTED, "deferred weight decay needs row_len % 4 == 0 and 16-byte aligned tables");
    return OKGE_OK;
}

// (written so that a NaN fails every comparison it takes part in)
int check_adam_hyper(float lr, float beta1, float beta2, float eps)
{
    if (!(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f && lr >= 0.f))
        return fail(OKGE_ERR_INVALID, "adam needs 0 <= beta1, beta2 < 1, eps >= 0 and lr >= 0");
    return OKGE_OK;
}

int lazy_tensor_dev(const okge_lazy_tensor &t, LazySeg &sg)
{
    if (!t.p || !t.g || !t.state_sum || t.rows < 0 || t.row_len <= 0) return fail(OKGE_ERR_INVALID, "bad lazy adagrad tensor");
    if (t.row_steps) {
        if (t.row_len % 4 || t.rows > INT32_MAX) return fail(OKGE_ERR_INVALID, "deferred rows need a row length that is a multiple of 4 and fewer than 2^31 rows");
        if (!aligned16(t.p, t.g, t.state_sum)) return fail(OKGE_ERR_INVALID, "adagrad buffers must be 16-byte aligned");
        if (int rc = check_stamp(t.row_touched, t.touched_stamp)) return rc;
    } else if (t.row_touched) return fail(OKGE_ERR_INVALID, "a touched-row map needs row_steps");
    sg = LazySeg{t.p, t.g, t.state_sum, t.row_steps, t.row_touched, t.rows, t.row_len, t.touched_stamp};
    return OKGE_OK;
}

}  // namespace

extern "C" {

int okge_scale_inplace(float *x, int64_t n, const float *alpha_dev, void *stream)
{
    if (!x || !alpha_dev || n < 0) return fail(OKGE_ERR_INVALID, "bad scale arguments");
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("scale", "scale", st, launch_scale(x, n, alpha_dev, st));
}

int okge_rescale_gradients(float *g0, int64_t n0, float *g1, int64_t n1, const float *alpha_dev, float applied, void *stream)
{
    if (!g0 || !alpha_dev || n0 < 0 || n1 < 0 || (n1 > 0 && !g1) || !(applied > 0.f))
        return fail(OKGE_ERR_INVALID, "bad rescale arguments");
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("rescale", "rescale", st, launch_rescale2(g0, n0, g1 ? g1 : g0, g1 ? n1 : 0, alpha_dev, applied, st));
}

int okge_adagrad_step(float *p, float *g, float *state_sum, int64_t n, float lr, float weight_decay, float eps,
                      int32_t zero_grad, void *stream)
{
    if (int rc = check_adagrad(p, g, state_sum, n)) return rc;
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("adagrad", "adagrad", st, launch_adagrad(p, g, state_sum, n, lr, weight_decay, eps, zero_grad, st));
}

int okge_adagrad_step2(float *p0, float *g0, float *sum0, int64_t n0, float *p1, float *g1, float *sum1, int64_t n1,
                       float lr, float weight_decay, float eps, int32_t zero_grad, void *stream)
{
    if (!p0 || !g0 || !sum0 || n0 < 0 || !p1 || !g1 || !sum1 || n1 < 0)
        return fail(OKGE_ERR_INVALID, "bad adagrad arguments");
    if (!aligned16(p0, g0, sum0, p1, g1, sum1)) return fail(OKGE_ERR_INVALID, "adagrad buffers must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("adagrad", "adagrad", st, launch_adagrad2(p0, g0, sum0, n0, p1, g1, sum1, n1, lr, weight_decay, eps, zero_grad, st));
}

int okge_adagrad_multi(const okge_adagrad_tensor *tensors, int32_t n_tensors, float lr, float weight_decay, float eps, void *stream)
{
    if (!tensors || n_tensors <= 0 || n_tensors > ADAGRAD_MAX_SEGS) return fail(OKGE_ERR_INVALID, "1 to 4 tensors per adagrad launch");
    AdagradSegM segs[ADAGRAD_MAX_SEGS];
    for (int i = 0; i < n_tensors; ++i) {
        const okge_adagrad_tensor &t = tensors[i];
        if (int rc = check_adagrad(t.p, t.g, t.state_sum, t.n)) return rc;
        if (t.row_touched) {
            if (int rc = check_touched_rows(t.row_touched, t.row_len, t.touched_stamp, t.n)) return rc;
            if (!t.zero_grad) return fail(OKGE_ERR_INVALID, "a touched-row map needs zero_grad (rows not stamped must hold zero gradients)");
        }
        segs[i] = AdagradSegM{t.p, t.g, t.state_sum, t.n, t.row_touched, t.row_len, t.touched_stamp, t.zero_grad};
    }
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("adagrad", "adagrad", st, launch_adagrad_multi(segs, n_tensors, lr, weight_decay, eps, st));
}

// ---- okge_adagrad_rows: torch's sparse Adagrad on occurrence rows ---------------------------------------------------------------
size_t okge_adagrad_rows_workspace_bytes(int64_t n0, int64_t n1)
{
    if (n0 < 0 || n1 < 0 || n0 > ROWS_MAX_N || n1 > ROWS_MAX_N) return 0;
    Arena ar;
    if (n0 > 0) take_rows_keys(ar, n0);
    if (n1 > 0) take_rows_keys(ar, n1);
    return ar.total();
}

int okge_adagrad_rows(const okge_rows_tensor *tensors, int32_t n_tensors, float lr, float eps, void *workspace, size_t workspace_bytes,
                      void *stream)
{
    if (int rc = check_rows_count(tensors, n_tensors, 0)) return rc;
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
    hipStream_t st = as_stream(stream);
    int sorted_in = 0;
    if (int rc = rows_sort(segs, &sorted_in, st)) return rc;
    return OKGE_TIMED("rows_update", "rows_update", st, launch_rows_update(segs, sorted_in, lr, eps, st));
}

// ---- okge_rows_to_dense: the occurrence rows coalesced into dense gradient tables, order fixed ----------------------------------
size_t okge_rows_to_dense_workspace_bytes(int64_t n0, int64_t n1) { return okge_adagrad_rows_workspace_bytes(n0, n1); }

int okge_rows_to_dense(const okge_rows_tensor *tensors, int32_t n_tensors, int32_t mode, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = check_rows_count(tensors, n_tensors, 0)) return rc;
    if (mode != OKGE_ROWS_STORE && mode != OKGE_ROWS_ACCUMULATE) return fail(OKGE_ERR_INVALID, "mode is OKGE_ROWS_STORE or OKGE_ROWS_ACCUMULATE");
    Arena need;
    for (int k = 0; k < n_tensors; ++k) {
        const okge_rows_tensor &x = tensors[k];
        if (x.n < 0) return fail(OKGE_ERR_INVALID, "negative occurrence count");
        if (x.n > ROWS_MAX_N) return fail(OKGE_ERR_UNSUPPORTED, "okge_rows_to_dense takes up to 2^20 occurrence rows per tensor");
        if (x.n == 0) continue;
        if (!x.p || !x.ids || !x.g) return fail(OKGE_ERR_INVALID, "null tensor");
        if (x.table_rows <= 0 || x.row_len <= 0 || x.ld_g < x.row_len) return fail(OKGE_ERR_INVALID, "bad table shape / leading dimension");
        take_rows_keys(need, x.n);
    }
    if (need.total() == 0) return OKGE_OK;
    if (!workspace || workspace_bytes < need.total()) return fail(OKGE_ERR_WORKSPACE, "workspace too small (okge_rows_to_dense_workspace_bytes)");
    RowsSegs segs;
    std::memset(&segs, 0, sizeof(segs));
    char *ws = static_cast<char *>(workspace);
    Arena ar;
    for (int k = 0; k < n_tensors; ++k) {
        const okge_rows_tensor &x = tensors[k];
        if (x.n > 0) rows_segment(segs, ws, ar, x.p, nullptr, x.ids, x.g, x.ld_g, x.n, x.table_rows, x.row_len, nullptr);   // (state_sum is not read)
    }
    segs.id_err = id_err_ptr();
    hipStream_t st = as_stream(stream);
    int sorted_in = 0;
    if (int rc = rows_sort(segs, &sorted_in, st)) return rc;
    return OKGE_TIMED("rows_to_dense", "rows_to_dense", st, launch_rows_to_dense(segs, sorted_in, mode == OKGE_ROWS_ACCUMULATE, st));
}

// ---- Adam: torch.optim.Adam's dense update and torch.optim.SparseAdam's on occurrence rows --------------------------------------
int okge_adam_step(const okge_adam_tensor *tensors, int32_t n_tensors, float lr, float beta1, float beta2, float eps, float weight_decay,
                   int32_t zero_grad, void *stream)
{
    if (!tensors || n_tensors < 1 || n_tensors > ADAM_MAX_SEGS) return fail(OKGE_ERR_INVALID, "one or two tensors");
    AdamSeg segs[ADAM_MAX_SEGS] = {};
    int32_t *states[ADAM_MAX_SEGS] = {};
    for (int k = 0; k < n_tensors; ++k) {
        const okge_adam_tensor &x = tensors[k];
        if (!x.p || !x.g || !x.exp_avg || !x.exp_avg_sq || !x.state || x.n < 0) return fail(OKGE_ERR_INVALID, "bad adam arguments");
        if (!aligned16(x.p, x.g, x.exp_avg, x.exp_avg_sq)) return fail(OKGE_ERR_INVALID, "adam buffers must be 16-byte aligned");
        segs[k] = AdamSeg{x.p, x.g, x.exp_avg, x.exp_avg_sq, x.state, x.n};
        states[k] = x.state;
    }
    if (int rc = check_adam_hyper(lr, beta1, beta2, eps)) return rc;
    if (!(weight_decay >= 0.f)) return fail(OKGE_ERR_INVALID, "adam needs weight_decay >= 0");
    if (zero_grad < 0 || zero_grad > 2) return fail(OKGE_ERR_INVALID, "zero_grad is 0 (none), 1 (both) or 2 (second tensor only)");
    hipStream_t st = as_stream(stream);
    if (int rc = OKGE_TIMED("adam_prologue", "adam_prologue", st, launch_adam_prologue(states, n_tensors, lr, beta1, beta2, st))) return rc;
    return OKGE_TIMED("adam", "adam", st, launch_adam2(segs[0], segs[1], beta1, beta2, eps, weight_decay, zero_grad, st));
}

int okge_adam_multi(const okge_adam_multi_tensor *tensors, int32_t n_tensors, float lr, float beta1, float beta2, float eps,
                    float weight_decay, void *stream)
{
    if (!tensors || n_tensors < 1 || n_tensors > ADAM_MULTI_MAX_SEGS) return fail(OKGE_ERR_INVALID, "1 to 4 tensors per adam launch");
    AdamSegM segs[ADAM_MULTI_MAX_SEGS] = {};
    int32_t *states[ADAM_MULTI_MAX_SEGS] = {};
    for (int k = 0; k < n_tensors; ++k) {
        const okge_adam_multi_tensor &x = tensors[k];
        if (!x.p || !x.g || !x.exp_avg || !x.exp_avg_sq || !x.state || x.n < 0) return fail(OKGE_ERR_INVALID, "bad adam arguments");
        if (!aligned16(x.p, x.g, x.exp_avg, x.exp_avg_sq)) return fail(OKGE_ERR_INVALID, "adam buffers must be 16-byte aligned");
        if (int rc = check_touched_rows(x.row_touched, x.row_len, x.touched_stamp, x.n)) return rc;
        segs[k] = AdamSegM{x.p, x.g, x.exp_avg, x.exp_avg_sq, x.state, x.n, x.row_touched, x.row_len, x.touched_stamp};
        states[k] = x.state;
    }
    if (int rc = check_adam_hyper(lr, beta1, beta2, eps)) return rc;
    if (!(weight_decay >= 0.f)) return fail(OKGE_ERR_INVALID, "adam needs weight_decay >= 0");
    hipStream_t st = as_stream(stream);
    if (int rc = OKGE_TIMED("adam_prologue", "adam_prologue", st, launch_adam_prologue(states, n_tensors, lr, beta1, beta2, st))) return rc;
    return OKGE_TIMED("adam", "adam_multi", st, launch_adam_multi(segs, n_tensors, beta1, beta2, eps, weight_decay, st));
}

size_t okge_adam_rows_workspace_bytes(int64_t n0, int64_t n1) { return okge_adagrad_rows_workspace_bytes(n0, n1); }

int okge_adam_rows(const okge_adam_rows_tensor *tensors, int32_t n_tensors, float lr, float beta1, float beta2, float eps, void *workspace,
                   size_t workspace_bytes, void *stream)
{
    if (int rc = check_rows_count(tensors, n_tensors, 1)) return rc;
    Arena need;
    int32_t *states[ROWS_MAX_SEGS] = {};
    for (int k = 0; k < n_tensors; ++k) {
        const okge_adam_rows_tensor &x = tensors[k];
        if (x.n < 0) return fail(OKGE_ERR_INVALID, "negative occurrence count");
        if (x.n > ROWS_MAX_N) return fail(OKGE_ERR_UNSUPPORTED, "okge_adam_rows takes up to 2^20 occurrence rows per tensor");
        if (!x.state) return fail(OKGE_ERR_INVALID, "null tensor");          // (t advances whatever n is)
        states[k] = x.state;
        if (x.n == 0) continue;
        if (!x.p || !x.exp_avg || !x.exp_avg_sq || !x.ids || !x.g) return fail(OKGE_ERR_INVALID, "null tensor");
        if (x.table_rows <= 0 || x.row_len <= 0 || x.ld_g < x.row_len) return fail(OKGE_ERR_INVALID, "bad table shape / leading dimension");
        take_rows_keys(need, x.n);
    }
    if (int rc = check_adam_hyper(lr, beta1, beta2, eps)) return rc;
    if (need.total() && (!workspace || workspace_bytes < need.total()))
        return fail(OKGE_ERR_WORKSPACE, "workspace too small (okge_adam_rows_workspace_bytes)");
    RowsSegs segs;
    std::memset(&segs, 0, sizeof(segs));
    char *ws = static_cast<char *>(workspace);
    Arena ar;
    for (int k = 0; k < n_tensors; ++k) {
        const okge_adam_rows_tensor &x = tensors[k];
        if (x.n > 0) rows_segment(segs, ws, ar, x.p, x.exp_avg, x.ids, x.g, x.ld_g, x.n, x.table_rows, x.row_len, nullptr, x.exp_avg_sq, x.state);
    }
    hipStream_t st = as_stream(stream);
    // SparseAdam.step counts the step before it skips an empty gradient: every tensor's t advances, whatever its n
    if (int rc = OKGE_TIMED("adam_prologue", "adam_prologue", st, launch_adam_prologue(states, n_tensors, lr, beta1, beta2, st))) return rc;
    if (!segs.n_segs) return OKGE_OK;
    segs.id_err = id_err_ptr();
    int sorted_in = 0;
    if (int rc = rows_sort(segs, &sorted_in, st)) return rc;
    return OKGE_TIMED("rows_update_adam", "rows_update_adam", st, launch_rows_update_adam(segs, sorted_in, beta1, beta2, eps, st));
}

int okge_rows_catch_up(const okge_rows_decay_tensor *tensors, int32_t n_tensors, const int32_t *counters, float lr, float weight_decay,
                       float eps, void *stream)
{
    if (int rc = check_rows_count(tensors, n_tensors, 0)) return rc;
    if (!counters) return fail(OKGE_ERR_INVALID, "okge_rows_catch_up needs the counters");
    RowsCatchSeg segs[ROWS_MAX_SEGS];
    for (int k = 0; k < n_tensors; ++k) {
        const okge_rows_decay_tensor &x = tensors[k];
        if (int rc = rows_decay_table(x, "okge_rows_catch_up")) return rc;
        segs[k] = RowsCatchSeg{x.p, x.state_sum, x.row_steps, x.ids, x.n, x.table_rows, x.row_len, 0};
    }
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("rows_catch_up", "rows_catch_up", st, launch_rows_catch_up(segs, n_tensors, counters, lr, weight_decay, eps, st));
}

int okge_adagrad_rows_decay(const okge_rows_decay_tensor *tensors, int32_t n_tensors, int32_t *counters, int32_t window, float lr,
                            float weight_decay, float eps, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = check_rows_count(tensors, n_tensors, 1)) return rc;
    if (!counters || window < 1) return fail(OKGE_ERR_INVALID, "okge_adagrad_rows_decay needs the counters and window >= 1");
    Arena need;
    for (int k = 0; k < n_tensors; ++k) {
        const okge_rows_decay_tensor &x = tensors[k];
        if (int rc = rows_decay_table(x, "okge_adagrad_rows_decay")) return rc;
        if (x.n == 0) continue;
        if (!x.g || x.ld_g < x.row_len) return fail(OKGE_ERR_INVALID, "null gradient rows / bad leading dimension");
        if (x.ld_g % 4 || !aligned16(x.g))
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
    hipStream_t st = as_stream(stream);
    if (segs.n_segs) {
        int sorted_in = 0;
        if (int rc = rows_sort(segs, &sorted_in, st)) return rc;
        if (int rc = OKGE_TIMED("rows_update", "rows_update_decay", st,
                                launch_rows_update_decay(segs, sorted_in, counters, lr, weight_decay, eps, st))) return rc;
    }
    // the due slice -- rows with r % window == T % window that the update above did not bring to T + 1 -- and T += 1 on the device
    return OKGE_TIMED("rows_decay_sweep", "rows_decay_sweep", st,
                      launch_adagrad_lazy(sweep, n_tensors, counters, window, LAZY_STEP, lr, weight_decay, eps, st));
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
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED(mode == OKGE_LAZY_STEP ? "adagrad" : "adagrad_flush", "adagrad_lazy", st,
                      launch_adagrad_lazy(segs, n_tensors, counters, window, mode, lr, weight_decay, eps, st));
}

int okge_pool_catch_up_calls(const okge_pool_call *calls, int32_t n_calls, const okge_lazy_tensor *tables, int32_t n_tables,
                             const int32_t *counters, float lr, float weight_decay, float eps, void *stream)
{
    if (int rc = check_pool_calls(calls, n_calls)) return rc;
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
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("pool_catch_up", "pool_catch_up", st, launch_pool_catch_up(q, nq, counters, lr, weight_decay, eps, id_err_ptr(), st));
}

int okge_clip_grad_norm(float *g0, int64_t n0, float *g1, int64_t n1, float max_norm, double *norm_out_dev, void *workspace,
                        size_t workspace_bytes, void *stream)
{
    if (!g0 || n0 < 0 || n1 < 0 || (n1 > 0 && !g1) || !(max_norm > 0.f)) return fail(OKGE_ERR_INVALID, "bad clip_grad_norm arguments");
    constexpr int NP = 1024;
    if (!workspace || workspace_bytes < NP * sizeof(double) + 256) return fail(OKGE_ERR_WORKSPACE, "workspace too small (8448 bytes)");
    hipStream_t st = as_stream(stream);
    double *partial = static_cast<double *>(workspace);
    float *coef = reinterpret_cast<float *>(static_cast<char *>(workspace) + NP * sizeof(double));
    hipError_t e;
    {
        ScopedTimer tm("clip_grad_norm", st);       // the coefficient and the scaling under one name
        if (int rc = hip_ok(launch_clip_coef(g0, n0, g1 ? g1 : g0, g1 ? n1 : 0, max_norm, partial, NP, coef, norm_out_dev, st), "clip_coef"))
            return rc;
        e = launch_scale(g0, n0, coef, st);
        if (e == hipSuccess && g1 && n1 > 0) e = launch_scale(g1, n1, coef, st);
    }
    return hip_ok(e, "scale gradients");
}

constexpr int CLIP_MULTI_PARTIALS = 1024;       // the fixed grid of the partial sums

size_t okge_clip_grad_norm_multi_workspace_bytes(void) { return CLIP_MULTI_PARTIALS * sizeof(double) + 256; }

int okge_clip_grad_norm_multi(const okge_grad_tensor *tensors, int32_t n_tensors, float max_norm, double *norm_out_dev, void *workspace,
                              size_t workspace_bytes, void *stream)
{
    if (!tensors || n_tensors < 1 || n_tensors > CLIP_MAX_SEGS) return fail(OKGE_ERR_INVALID, "1 to 8 tensors per clip_grad_norm launch");
    GradSeg segs[CLIP_MAX_SEGS] = {};
    for (int k = 0; k < n_tensors; ++k) {
        const okge_grad_tensor &x = tensors[k];
        if (!x.g || x.n < 0) return fail(OKGE_ERR_INVALID, "bad clip_grad_norm arguments");
        if (int rc = check_touched_rows(x.row_touched, x.row_len, x.touched_stamp, x.n)) return rc;
        if (x.row_touched && !aligned16(x.g)) return fail(OKGE_ERR_INVALID, "gradient rows under a touched-row map must be 16-byte aligned");
        segs[k] = GradSeg{x.g, x.n, x.row_touched, x.row_len, x.touched_stamp};
    }
    if (!(max_norm > 0.f)) return fail(OKGE_ERR_INVALID, "clip_grad_norm needs max_norm > 0");
    if (!workspace || workspace_bytes < okge_clip_grad_norm_multi_workspace_bytes())
        return fail(OKGE_ERR_WORKSPACE, "workspace too small (okge_clip_grad_norm_multi_workspace_bytes)");
    hipStream_t st = as_stream(stream);
    double *partial = static_cast<double *>(workspace);
    float *coef = reinterpret_cast<float *>(static_cast<char *>(workspace) + CLIP_MULTI_PARTIALS * sizeof(double));
    return OKGE_TIMED("clip_grad_norm", "clip_grad_norm_multi", st,
                      launch_clip_multi(segs, n_tensors, max_norm, partial, CLIP_MULTI_PARTIALS, coef, norm_out_dev, st));
}

int okge_merge_logsumexp(const float *parts, int32_t world, int32_t B, float *out, void *stream)
{
    if (!parts || !out || world <= 0 || B <= 0) return fail(OKGE_ERR_INVALID, "bad merge_logsumexp arguments");
    hipStream_t st = as_stream(stream);
    return OKGE_TIMED("merge_lse", "merge_lse", st, launch_merge_lse(parts, world, B, out, st));
}

}  // extern "C"
