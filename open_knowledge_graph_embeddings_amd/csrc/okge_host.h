// What the host-side translation units of the C ABI (okge_core.hip, okge_api_*.hip) share: the error path, HIP-event timing,
// the per-device state, the descriptor conversions and the argument checks more than one family runs.  Host only; the
// definitions and all of the state live in okge_core.hip unless a line says otherwise.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <string>

#include "../../include/okge.h"
#include "okge_kernels.h"
#include "okge_plan.h"

#pragma GCC visibility push(hidden)
namespace okge {

int fail(int code, const std::string &msg);          // sets okge_last_error() (thread-local), returns code
int fail_hip(hipError_t e, const char *what);        // "<what>: <HIP error string>", OKGE_ERR_HIP
inline int hip_ok(hipError_t e, const char *what) { return e == hipSuccess ? OKGE_OK : fail_hip(e, what); }

inline hipStream_t as_stream(void *stream) { return reinterpret_cast<hipStream_t>(stream); }

// ---- per-kernel HIP-event timing (okge_timing_*) ------------------------------------------------------------------------------
struct TimedLaunch {
    const char *name;
    hipEvent_t  start, stop;
};
extern bool g_timing;           // okge_timing_enable
struct ScopedTimer {
    hipStream_t st;
    bool        on;
    TimedLaunch t;
    ScopedTimer(const char *name, hipStream_t s) : st(s), on(g_timing) { if (on) start(name); }
    ~ScopedTimer() { if (on) stop(); }
    void start(const char *name);
    void stop();
};
// the launches `launch()` issues under the timer `timer`; a failure reads "<what>: ...".  Returns OKGE_OK or the error code
template <class Launch>
int timed(const char *timer, const char *what, hipStream_t st, Launch &&launch)
{
    ScopedTimer tm(timer, st);
    return hip_ok(launch(), what);
}
// the usual case, one launch expression:  if (int rc = OKGE_TIMED("dq", "dq_kernel", st, launch_dq(q, grid, st))) return rc;
#define OKGE_TIMED(timer, what, st, launch) ::okge::timed(timer, what, st, [&] { return launch; })

// ---- per-device state --------------------------------------------------------------------------------------------------------
constexpr int OKGE_MAX_DEVICES = 64;
extern std::mutex g_dev_mu;     // guards the per-device tables (id-error words; the evaluation pipeline's event sets)
int  current_device();          // hipGetDevice(), or -1
int *id_err_ptr();              // device word counting out-of-range ids (checked_row in the kernels); okge_id_errors reads and clears it
int  cu_count();                // compute units of the current device; 256 where no device answers.  The planner takes it as an argument

// ---- descriptors -> what the kernels take --------------------------------------------------------------------------------------
DropDev   to_dev(const okge_dropout &d);
PrefixDev to_dev(const okge_prefix_batch &b, const okge_tables *t, const okge_shard *sh = nullptr);

// ---- checks ------------------------------------------------------------------------------------------------------------------
bool known_scorer(int32_t scorer);
int  refuse_bias(int32_t scorer, const char *entry, const char *why);
// wide_ok: the entry point has a wide path (slot sizes 513 .. 4096); every other one stops at 512
int  check_common(const okge_tables *t, const okge_prefix_batch *b, const okge_candidates *c, bool wide_ok = false);
int  check_common(const okge_tables *t, const okge_prefix_batch *b);      // an entry point without candidates
int  check_shard(const okge_tables *t, const okge_shard *sh);
int  check_local_range(const okge_tables *t, const okge_candidates *c);   // sharded phases: a candidate range lies in the local table
bool any_dropout(const okge_prefix_batch *b, const okge_candidates *c);

template <class... T>
bool aligned16(const T *...p) { return ((reinterpret_cast<uintptr_t>(p) | ...) % 16) == 0; }
// a score block the sweep may store with 16-byte accesses
inline bool x_vec_ok(const float *scores, int64_t ld_scores) { return ld_scores % 4 == 0 && aligned16(scores); }

// ---- the tile sweep, which fused evaluation (okge_api_eval.hip) runs too: defined in okge_api_train.hip ---------------------
// the arguments every tile launch (slot sizes up to 512) shares; Q: the folded queries.  b_per_block: all rows
void       fill_fused_common(FusedArgs &a, const Shape &s, const okge_tables *t, const okge_candidates *c, const float *Q);
hipError_t launch_sweep(const Shape &s, const SweepPlan &p, const FusedArgs &a0, hipStream_t st, int mode = MODE_SCORE);

// ---- the token-pooled embedder's checks, which the optimizers' pool catch-up runs too: defined in okge_api_encoders.hip -----
int check_token_embedder(const okge_token_embedder *e, const int32_t *ids, int32_t first_id, int32_t n);
int check_pool_calls(const okge_pool_call *calls, int32_t n_calls);       // 1 to POOL_MAX_CALLS of them

}  // namespace okge
#pragma GCC visibility pop
