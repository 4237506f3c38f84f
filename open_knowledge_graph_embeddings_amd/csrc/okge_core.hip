// C ABI (include/okge.h) over the gfx950 kernels: the core of its host side (okge_host.h).  Error state, HIP-event timing, the
// per-device id-error word and CU count, the descriptor conversions and the shared argument checks; the entry points live in
// okge_api_*.hip, one unit per family.  Host-side only.  No torch, no CPU fallback: every entry point either enqueues HIP
// kernels or returns an error.
#include <vector>

#include "okge_host.h"

namespace okge {

static_assert(sizeof(v8bf) == PLANE_CELL_BYTES && sizeof(TopkRec) == TOPK_REC_BYTES, "okge_plan.h sizes its regions with these");

static thread_local std::string g_err;

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

int report_error(int code, const std::string &msg) { return fail(code, msg); }

// ---- per-kernel HIP-event timing ----------------------------------------------------------------------
static std::mutex               g_tmu;
bool                            g_timing = false;
static std::vector<TimedLaunch> g_launches;
static std::vector<hipEvent_t>  g_event_pool;

static hipEvent_t get_event()
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

void ScopedTimer::start(const char *name)
{
    std::lock_guard<std::mutex> lk(g_tmu);
    t.name = name;
    t.start = get_event();
    t.stop = get_event();
    (void)hipEventRecord(t.start, st);
}

void ScopedTimer::stop()
{
    (void)hipEventRecord(t.stop, st);
    std::lock_guard<std::mutex> lk(g_tmu);
    g_launches.push_back(t);
}

// ---- device word counting out-of-range ids (checked_row in the kernels); read and cleared by okge_id_errors ------------
// One word PER DEVICE (keyed by hipGetDevice() at the call): a process that drives several devices must never hand a kernel
// on device b a pointer that lives on device a.
std::mutex g_dev_mu;
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

PrefixDev to_dev(const okge_prefix_batch &b, const okge_tables *t, const okge_shard *sh)
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

bool known_scorer(int32_t scorer)
{
    return scorer == OKGE_COMPLEX || scorer == OKGE_DISTMULT || scorer == OKGE_BIAS_RELATION || scorer == OKGE_BIAS_ENTITY;
}
static const char *scorer_name(int32_t scorer) { return scorer == OKGE_BIAS_RELATION ? "OKGE_BIAS_RELATION" : "OKGE_BIAS_ENTITY"; }
// the data-bias scorers (model.py:281-350) score prefixes only and leave one slot without a gradient: the entry points that
// score triples, step every table or fold from exchanged entity rows refuse them before anything is written
int refuse_bias(int32_t scorer, const char *entry, const char *why)
{
    if (scorer != OKGE_BIAS_RELATION && scorer != OKGE_BIAS_ENTITY) return OKGE_OK;
    return fail(OKGE_ERR_UNSUPPORTED, std::string(entry) + " does not take the " + scorer_name(scorer) + " scorer: " + why);
}

// wide_ok: the entry point has a wide path (slot sizes 513 .. 4096: okge_score_prefixes, okge_train_forward_backward,
// okge_evaluate_batch); every other one stops at 512
int check_common(const okge_tables *t, const okge_prefix_batch *b, const okge_candidates *c, bool wide_ok)
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

// an entry point without candidates: one candidate that passes stands in
int check_common(const okge_tables *t, const okge_prefix_batch *b)
{
    okge_candidates none;
    std::memset(&none, 0, sizeof(none));
    none.n = 1; none.first_id = 0;
    return check_common(t, b, &none);
}

int check_shard(const okge_tables *t, const okge_shard *sh)
{
    if (!sh) return fail(OKGE_ERR_INVALID, "null shard descriptor");
    if (sh->ent_lo < 0 || sh->ent_hi <= sh->ent_lo || sh->ent_hi - sh->ent_lo != t->n_ent)
        return fail(OKGE_ERR_INVALID, "shard range must cover exactly the rows of the local entity table");
    return OKGE_OK;
}

int check_local_range(const okge_tables *t, const okge_candidates *c)
{
    if (!c->ids && (c->first_id < 0 || (int64_t)c->first_id + c->n > t->n_ent))
        return fail(OKGE_ERR_INVALID, "candidate range outside the local entity table");
    return OKGE_OK;
}

bool any_dropout(const okge_prefix_batch *b, const okge_candidates *c)
{
    return c->drop.p > 0.f || (b && (b->drop_po_ent.p > 0.f || b->drop_po_rel.p > 0.f || b->drop_sp_ent.p > 0.f || b->drop_sp_rel.p > 0.f));
}

}  // namespace okge

using namespace okge;

extern "C" {

int okge_abi_version(void) { return OKGE_ABI_VERSION; }

const char *okge_last_error(void) { return g_err.c_str(); }

int okge_id_errors(int64_t *n_out)
{
    int *p = id_err_ptr();
    if (!p || !n_out) return fail(OKGE_ERR_INVALID, "no id error word");
    int v = 0;
    // (synchronises: call it when you would sync anyway)
    if (int rc = hip_ok(hipMemcpy(&v, p, sizeof(int), hipMemcpyDeviceToHost), "read id error word")) return rc;
    if (v)
        if (int rc = hip_ok(hipMemset(p, 0, sizeof(int)), "clear id error word")) return rc;
    *n_out = v;
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

// (timer names are compared as text: the same literal in two translation units need not be one address)
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
            if (std::strcmp(names[i], t.name) == 0) break;
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
