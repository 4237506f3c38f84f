// Row-sparse training of the lookup models (model_config.sparse: nn.Embedding(sparse=True) + torch's sparse Adagrad,
// model.py:390-391).  Kernels of
//   okge_train_forward_backward(OKGE_TRAIN_ROW_GRADS)   rows_gather_kernel: the occurrence rows of one batch as two small tables
//   okge_adagrad_rows                                   rows_sort_chunk_kernel / rows_merge_kernel: occurrences ordered by (id, position)
//                                                       rows_update_kernel<AdagradRows>: per distinct id, its gradient rows added up in
//                                                       ascending position, sequentially in fp32, then the Adagrad update of that table row
//   okge_rows_catch_up                                  rows_catch_up_kernel: the rows a batch names take the decay-only steps they owe
//   okge_adagrad_rows_decay                             rows_update_decay_kernel: the same walk with the weight-decay term, per-row step
//                                                       counters kept (deferred weight decay; the rotating sweep is okge_optim.hip's)
//   okge_adam_rows                                      rows_update_kernel<AdamRows>: the same sort and walk, torch's sparse Adam on the row
//   okge_rows_to_dense                                  rows_update_kernel<DenseRows<ACC>>: the same sort and walk, the coalesced row written to
//                                                       (ACC: continued from) the row of a DENSE gradient table -- the order-fixed dense gradient
// Nothing here is proportional to the table: the sort is O(n log n) on 8-byte keys, the update touches the n gradient rows and
// the distinct table rows they name.  No float atomics, no host synchronisation; the launch sequence depends on the n alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "okge_kernels.h"
#include "okge_adagrad_device.h"
#include "okge_adam_device.h"

namespace okge {

namespace {

constexpr int SORT_CHUNK = 1024;          // keys one workgroup orders in LDS (bitonic network, one compare-exchange per thread and step)
constexpr int MERGE_PER_THREAD = 4;       // outputs one thread of a merge pass produces
constexpr uint64_t KEY_SKIP = ~0ull;      // an occurrence whose id lies outside the table: sorts behind every real key, never written

__device__ __forceinline__ void copy_row(const float *__restrict__ src, float *__restrict__ dst, int d, int vec)
{
    if (vec) {
        const float4 *s4 = reinterpret_cast<const float4 *>(src);
        float4 *d4 = reinterpret_cast<float4 *>(dst);
        for (int k = threadIdx.x; k < (d >> 2); k += blockDim.x) d4[k] = s4[k];
    } else {
        for (int k = threadIdx.x; k < d; k += blockDim.x) dst[k] = src[k];
    }
}

// block r < N: candidate r; N <= r < N + B: prefix entity of batch row r - N; then: relation of batch row r - N - B
// (po rows first, as everywhere).  The position ids the relabelled problem names its rows by are written alongside.
__global__ __launch_bounds__(64) void rows_gather_kernel(const RowsGather a)
{
    const int r = blockIdx.x, B = a.n_po + a.n_sp;
    int *err = threadIdx.x == 0 ? a.id_err : nullptr;
    if (r < a.N) {
        const int64_t row = checked_row(a.cand_ids ? (int64_t)a.cand_ids[r] : (int64_t)a.cand_first + r, a.n_ent, err);
        copy_row(a.E + row * a.d, a.EV + (size_t)r * a.d, a.d, a.vec);
    } else if (r < a.N + B) {
        const int i = r - a.N;
        const int64_t row = checked_row(i < a.n_po ? a.po_obj[i] : a.sp_subj[i - a.n_po], a.n_ent, err);
        copy_row(a.E + row * a.d, a.EV + (size_t)r * a.d, a.d, a.vec);
        if (threadIdx.x == 0) a.pos_ids[i] = r;
    } else {
        const int i = r - a.N - B;
        const int64_t row = checked_row(i < a.n_po ? a.po_rel[i] : a.sp_rel[i - a.n_po], a.n_rel, err);
        copy_row(a.R + row * a.d, a.RV + (size_t)i * a.d, a.d, a.vec);
        if (threadIdx.x == 0) a.pos_ids[B + i] = i;
    }
}

// keys (id << 32 | position) of one chunk of occurrences, ordered: positions are distinct, so the order is total and "stable"
__global__ __launch_bounds__(SORT_CHUNK / 2) void rows_sort_chunk_kernel(const RowsSegs segs)
{
    const RowsSeg &sg = segs.s[blockIdx.y];
    __shared__ uint64_t k[SORT_CHUNK];
    const int base = blockIdx.x * SORT_CHUNK, tid = threadIdx.x;
    if (base >= sg.n) return;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int t = tid + h * (SORT_CHUNK / 2), i = base + t;
        uint64_t key = KEY_SKIP;
        if (i < sg.n) {
            const int32_t id = sg.ids[i];
            if ((uint32_t)id < (uint32_t)sg.table_rows) key = ((uint64_t)(uint32_t)id << 32) | (uint32_t)i;
            else if (segs.id_err) atomicAdd(segs.id_err, 1);
        }
        k[t] = key;
    }
    __syncthreads();
    for (int size = 2; size <= SORT_CHUNK; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const int lo = 2 * tid - (tid & (stride - 1));
            const bool up = (lo & size) == 0;
            const uint64_t x = k[lo], y = k[lo + stride];
            if ((x > y) == up) { k[lo] = y; k[lo + stride] = x; }
            __syncthreads();
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int t = tid + h * (SORT_CHUNK / 2);
        if (base + t < sg.n) sg.keys[0][base + t] = k[t];
    }
}

// one pass of the merge sort: ordered runs of `run` keys are merged in pairs, src -> dst; every thread finds its cut of the
// pair by bisection along its diagonal (merge path) and emits MERGE_PER_THREAD keys.  A run without a partner is copied.
__global__ __launch_bounds__(256) void rows_merge_kernel(const RowsSegs segs, int run, int from)
{
    const RowsSeg &sg = segs.s[blockIdx.y];
    const uint64_t *__restrict__ src = sg.keys[from];
    uint64_t *__restrict__ dst = sg.keys[from ^ 1];
    const int n = sg.n;
    const int out0 = (blockIdx.x * 256 + threadIdx.x) * MERGE_PER_THREAD;
    if (out0 >= n) return;
    const int base = out0 / (2 * run) * (2 * run);
    const int a_end = min(base + run, n), b_end = min(base + 2 * run, n);
    const uint64_t *A = src + base, *Bk = src + a_end;
    const int len_a = a_end - base, len_b = b_end - a_end, diag = out0 - base;
    int lo = max(0, diag - len_b), hi = min(diag, len_a);
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (A[mid] < Bk[diag - 1 - mid]) lo = mid + 1; else hi = mid;
    }
    int ia = lo, ib = diag - lo;
    for (int k = 0; k < MERGE_PER_THREAD && out0 + k < b_end; ++k) {
        const bool take_a = ib >= len_b || (ia < len_a && A[ia] < Bk[ib]);
        dst[out0 + k] = take_a ? A[ia++] : Bk[ib++];
    }
}

// V floats per access (4: 16-byte loads and stores; 1: row lengths / leading dimensions / bases that do not allow them).
// `lanes` lanes share the head of one run of equal ids: each walks the run for its columns, adding the gradient rows in
// ascending position, and updates its columns of the table row.  Runs are short in training batches (a candidate list names
// an entity once, a batch repeats a prefix entity a few times), so a lane's chain is a handful of dependent loads; several
// runs are in flight per wave (64 / lanes) and the waves of a CU hide the rest.
// The walk is stated once; what happens to the table row is the Body's: Body::Row<V> holds one column group of the row's state
// (loaded BEFORE the walk, so these loads are in flight while the gradient rows are added), takes the coalesced gradient and
// stores what it updated.
//   AdagradRows       adagrad1_rows, no decay term at all (okge_adagrad_rows)
//   AdagradRowsDecay  (V == 4 only; okge_adagrad_rows_decay) the row first takes the `lag` decay-only steps it still owes, then
//                     the update carries the weight-decay term -- adagrad4, the dense sweep's expression
//   AdamRows          adam1_rows (okge_adam_rows): two moment rows, the step size from the segment's device state
//   DenseRows<ACC>    no update at all (okge_rows_to_dense): the coalesced row IS the result, stored to row `id` of the dense
//                     gradient table sg.p.  ACC: the chain starts from the row the table holds -- (dE[id] + g_a) + g_b ..., not
//                     dE[id] + (g_a + g_b ...) -- which is what Row::first is for: it takes the run's first gradient row and
//                     returns the value the walk continues from (the other bodies return it as it is)
template <int V> struct RowVec { typedef float type; };
template <> struct RowVec<4> { typedef float4 type; };
template <int V> __device__ __forceinline__ typename RowVec<V>::type *row_ptr(float *x) { return reinterpret_cast<typename RowVec<V>::type *>(x); }
__device__ __forceinline__ void row_add(float &acc, float b) { acc += b; }
__device__ __forceinline__ void row_add(float4 &acc, const float4 &b) { acc.x += b.x; acc.y += b.y; acc.z += b.z; acc.w += b.w; }

struct AdagradRows {
    float lr, eps;
    template <int V> struct Row {
        typename RowVec<V>::type pv, sv;
        __device__ __forceinline__ void load(const RowsSeg &sg, size_t i) { pv = row_ptr<V>(sg.p)[i]; sv = row_ptr<V>(sg.s)[i]; }
        __device__ __forceinline__ typename RowVec<V>::type first(const typename RowVec<V>::type &g) const { return g; }
        __device__ __forceinline__ void update(const AdagradRows &b, const RowsSeg &, const typename RowVec<V>::type &acc)
        {
            if constexpr (V == 4) {
                adagrad1_rows(pv.x, acc.x, sv.x, b.lr, b.eps);
                adagrad1_rows(pv.y, acc.y, sv.y, b.lr, b.eps);
                adagrad1_rows(pv.z, acc.z, sv.z, b.lr, b.eps);
                adagrad1_rows(pv.w, acc.w, sv.w, b.lr, b.eps);
            } else {
                adagrad1_rows(pv, acc, sv, b.lr, b.eps);
            }
        }
        __device__ __forceinline__ void store(const RowsSeg &sg, size_t i) { row_ptr<V>(sg.p)[i] = pv; row_ptr<V>(sg.s)[i] = sv; }
    };
};

struct AdagradRowsDecay {
    float lr, wd, eps;
    int lag;
    template <int V> struct Row {
        float4 pv, sv;
        __device__ __forceinline__ void load(const RowsSeg &sg, size_t i) { pv = row_ptr<4>(sg.p)[i]; sv = row_ptr<4>(sg.s)[i]; }
        __device__ __forceinline__ float4 first(const float4 &g) const { return g; }
        __device__ __forceinline__ void update(const AdagradRowsDecay &b, const RowsSeg &, const float4 &acc)
        {
            // decay_replay4 votes across the wave.  Here the wave's lanes belong to different runs, lanes that are no head
            // of a run have returned and only the lanes of lagging rows enter (lag differs from run to run): the votes see
            // an arbitrary subset of the wave.  Both are used in the safe direction only -- "every active lane's operands
            // are ordinary" picks the short sqrt / div sequences, which return the generic bits on such operands, and one
            // lane that is not sends all to the generic code; "no active lane moved" skips steps that would return the bits
            // they were given, and one lane that moved makes the others repeat a step that changes nothing.  Either way
            // every lane ends with the bits of `lag` plain steps, whoever else took part in the vote.
            if (b.lag > 0) decay_replay4(pv, sv, b.lag, b.lr, b.wd, b.eps);
            adagrad4(pv, acc, sv, b.lr, b.wd, b.eps);
        }
        __device__ __forceinline__ void store(const RowsSeg &sg, size_t i) { row_ptr<4>(sg.p)[i] = pv; row_ptr<4>(sg.s)[i] = sv; }
    };
};

struct AdamRows {
    AdamHyper h;
    template <int V> struct Row {
        typename RowVec<V>::type pv, mv, vv;
        __device__ __forceinline__ void load(const RowsSeg &sg, size_t i)
        {
            pv = row_ptr<V>(sg.p)[i]; mv = row_ptr<V>(sg.s)[i]; vv = row_ptr<V>(sg.s2)[i];
        }
        __device__ __forceinline__ typename RowVec<V>::type first(const typename RowVec<V>::type &g) const { return g; }
        __device__ __forceinline__ void update(const AdamRows &b, const RowsSeg &sg, const typename RowVec<V>::type &acc)
        {
            const float step = __int_as_float(sg.state[ADAM_STEP]);
            if constexpr (V == 4) {
                adam1_rows(pv.x, acc.x, mv.x, vv.x, step, b.h);
                adam1_rows(pv.y, acc.y, mv.y, vv.y, step, b.h);
                adam1_rows(pv.z, acc.z, mv.z, vv.z, step, b.h);
                adam1_rows(pv.w, acc.w, mv.w, vv.w, step, b.h);
            } else {
                adam1_rows(pv, acc, mv, vv, step, b.h);
            }
        }
        __device__ __forceinline__ void store(const RowsSeg &sg, size_t i)
        {
            row_ptr<V>(sg.p)[i] = pv; row_ptr<V>(sg.s)[i] = mv; row_ptr<V>(sg.s2)[i] = vv;
        }
    };
};

template <bool ACC> struct DenseRows {
    template <int V> struct Row {
        typename RowVec<V>::type pv;
        __device__ __forceinline__ void load(const RowsSeg &sg, size_t i) { if constexpr (ACC) pv = row_ptr<V>(sg.p)[i]; }
        __device__ __forceinline__ typename RowVec<V>::type first(const typename RowVec<V>::type &g) const
        {
            if constexpr (ACC) {
                typename RowVec<V>::type acc = pv;
                row_add(acc, g);
                return acc;
            } else {
                return g;
            }
        }
        __device__ __forceinline__ void update(const DenseRows &, const RowsSeg &, const typename RowVec<V>::type &acc) { pv = acc; }
        __device__ __forceinline__ void store(const RowsSeg &sg, size_t i) { row_ptr<V>(sg.p)[i] = pv; }
    };
};

template <int V, class Body>
__device__ __forceinline__ void rows_update_run(const RowsSeg &sg, const uint64_t *__restrict__ keys, int i, uint32_t id, uint32_t pos,
                                                int lane, int lanes, const Body &body)
{
    typedef typename RowVec<V>::type vec_t;
    const int cols = sg.row_len / V;
    const int64_t ldg = sg.ld_g / V;
    const size_t prow = (size_t)id * cols;
    const vec_t *gv = reinterpret_cast<const vec_t *>(sg.g);
    for (int c = lane; c < cols; c += lanes) {
        typename Body::template Row<V> row;
        row.load(sg, prow + c);
        vec_t acc = row.first(gv[(size_t)pos * ldg + c]);
        for (int j = i + 1; j < sg.n; ++j) {
            const uint64_t kj = keys[j];
            if ((uint32_t)(kj >> 32) != id) break;
            row_add(acc, gv[(size_t)(uint32_t)kj * ldg + c]);
        }
        row.update(body, sg, acc);
        row.store(sg, prow + c);
    }
}

// the head of the run that thread (i, lane) works on, or false: past the end, an id outside the table (counted by the sort, never
// written), or not the first occurrence of its id
__device__ __forceinline__ bool rows_run_head(const RowsSeg &sg, const uint64_t *__restrict__ keys, int &i, int &lane, uint32_t &id, uint32_t &pos)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    i = t >> sg.lane_shift;
    lane = t & ((1 << sg.lane_shift) - 1);
    if (i >= sg.n) return false;
    const uint64_t key = keys[i];
    if (key == KEY_SKIP) return false;
    id = (uint32_t)(key >> 32);
    pos = (uint32_t)key;
    return !(i > 0 && (uint32_t)(keys[i - 1] >> 32) == id);
}

template <class Body>
__global__ __launch_bounds__(256) void rows_update_kernel(const RowsSegs segs, int sorted_in, const Body body)
{
    const RowsSeg &sg = segs.s[blockIdx.y];
    const uint64_t *__restrict__ keys = sg.keys[sorted_in];
    int i, lane;
    uint32_t id, pos;
    if (!rows_run_head(sg, keys, i, lane, id, pos)) return;
    if (sg.vec) rows_update_run<4>(sg, keys, i, id, pos, lane, 1 << sg.lane_shift, body);
    else rows_update_run<1>(sg, keys, i, id, pos, lane, 1 << sg.lane_shift, body);
}

// okge_adagrad_rows_decay: the same heads and the same walk; sg.vec holds by the entry point's preconditions.  T = the steps
// taken so far (counters[0], advanced by the sweep that follows this launch): a named row that still lags behind T -- the
// caller skipped okge_rows_catch_up -- replays what it owes first; every updated row then stands at T + 1.  One group of
// lanes owns a run, so nobody else reads or writes this row's counter; the group reads it before any of its lanes stores.
__global__ __launch_bounds__(256) void rows_update_decay_kernel(const RowsSegs segs, int sorted_in, const int32_t *__restrict__ counters,
                                                                float lr, float wd, float eps)
{
    const RowsSeg &sg = segs.s[blockIdx.y];
    const uint64_t *__restrict__ keys = sg.keys[sorted_in];
    int i, lane;
    uint32_t id, pos;
    if (!rows_run_head(sg, keys, i, lane, id, pos)) return;
    const int T = counters[0];
    const int lag = max(0, T - sg.steps[id]);
    rows_update_run<4>(sg, keys, i, id, pos, lane, 1 << sg.lane_shift, AdagradRowsDecay{lr, wd, eps, lag});
    if (lane == 0) sg.steps[id] = T + 1;
}

// Catch-up of the deferred decay-only steps before the forward gathers the rows (the scheme of pool_catch_up_kernel,
// okge_pool.hip).  Lane = occurrence: an id whose row lags behind T claims it with an integer atomicMax on the row's step
// counter -- the first claim wins, one owner per row however many occurrences name it -- then the wave replays its claimed rows,
// lane = column quad (lazy_rows).  Nothing in this launch reads a row it does not own; the gather runs in a later launch.
// ROWS_CATCH occurrences per wave and turn: many short waves, each with a handful of dependent row replays.
constexpr int ROWS_CATCH = 16;

__global__ __launch_bounds__(256, 5) void rows_catch_up_kernel(const RowsCatchSegs segs, const int32_t *__restrict__ counters, float lr, float wd,
                                                            float eps)
{
    const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= segs.wave0[segs.n_segs]) return;                                   // (the whole wave)
    int k = 0;
    while (gw >= segs.wave0[k + 1]) ++k;
    const RowsCatchSeg &sg = segs.s[k];
    const int T = counters[0], lane = threadIdx.x & 63;
    const int64_t i = (gw - segs.wave0[k]) * ROWS_CATCH + lane;
    int32_t id = -1;
    if (lane < ROWS_CATCH && i < sg.n) id = sg.ids[i];
    int from = T;
    bool claim = false;
    if ((uint32_t)id < (uint32_t)sg.table_rows && sg.steps[id] < T) {           // (ids outside the table: skipped here, counted by the sort)
        from = atomicMax(&sg.steps[id], T);
        claim = from < T;
    }
    lazy_rows(__ballot(claim), id, T - from, false, sg.p, sg.s, sg.s, sg.row_len, lane, lr, wd, eps);
}

}  // namespace

hipError_t launch_rows_gather(const RowsGather &a, hipStream_t st)
{
    const int rows = a.N + 2 * (a.n_po + a.n_sp);
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(rows_gather_kernel, dim3(rows), dim3(64), 0, st, a);
    return hipGetLastError();
}

// keys[0] / keys[1] of every segment: n keys each.  Returns in *sorted_in which of the two holds the ordered keys.
hipError_t launch_rows_sort(const RowsSegs &segs, int *sorted_in, hipStream_t st)
{
    int n_max = 0;
    for (int k = 0; k < segs.n_segs; ++k) n_max = std::max(n_max, segs.s[k].n);
    *sorted_in = 0;
    if (n_max <= 0) return hipSuccess;
    hipLaunchKernelGGL(rows_sort_chunk_kernel, dim3((n_max + SORT_CHUNK - 1) / SORT_CHUNK, segs.n_segs), dim3(SORT_CHUNK / 2), 0, st, segs);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    const int per_block = 256 * MERGE_PER_THREAD;
    for (int64_t run = SORT_CHUNK; run < n_max; run <<= 1) {                       // (a shorter segment's late passes are copies)
        hipLaunchKernelGGL(rows_merge_kernel, dim3((n_max + per_block - 1) / per_block, segs.n_segs), dim3(256), 0, st, segs, (int)run,
                           *sorted_in);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        *sorted_in ^= 1;
    }
    return hipSuccess;
}

hipError_t launch_rows_update(const RowsSegs &segs, int sorted_in, float lr, float eps, hipStream_t st)
{
    int64_t threads = 0;
    for (int k = 0; k < segs.n_segs; ++k) threads = std::max<int64_t>(threads, (int64_t)segs.s[k].n << segs.s[k].lane_shift);
    if (threads <= 0) return hipSuccess;
    hipLaunchKernelGGL(rows_update_kernel<AdagradRows>, dim3((unsigned)((threads + 255) / 256), segs.n_segs), dim3(256), 0, st, segs, sorted_in,
                       AdagradRows{lr, eps});
    return hipGetLastError();
}

hipError_t launch_rows_update_adam(const RowsSegs &segs, int sorted_in, float beta1, float beta2, float eps, hipStream_t st)
{
    int64_t threads = 0;
    for (int k = 0; k < segs.n_segs; ++k) {
        if (!segs.s[k].s2 || !segs.s[k].state) return hipErrorInvalidValue;
        threads = std::max<int64_t>(threads, (int64_t)segs.s[k].n << segs.s[k].lane_shift);
    }
    if (threads <= 0) return hipSuccess;
    hipLaunchKernelGGL(rows_update_kernel<AdamRows>, dim3((unsigned)((threads + 255) / 256), segs.n_segs), dim3(256), 0, st, segs, sorted_in,
                       AdamRows{adam_hyper(beta1, beta2, eps, 0.f)});
    return hipGetLastError();
}

hipError_t launch_rows_to_dense(const RowsSegs &segs, int sorted_in, int accumulate, hipStream_t st)
{
    int64_t threads = 0;
    for (int k = 0; k < segs.n_segs; ++k) threads = std::max<int64_t>(threads, (int64_t)segs.s[k].n << segs.s[k].lane_shift);
    if (threads <= 0) return hipSuccess;
    const dim3 grid((unsigned)((threads + 255) / 256), segs.n_segs);
    if (accumulate) hipLaunchKernelGGL(rows_update_kernel<DenseRows<true>>, grid, dim3(256), 0, st, segs, sorted_in, DenseRows<true>{});
    else hipLaunchKernelGGL(rows_update_kernel<DenseRows<false>>, grid, dim3(256), 0, st, segs, sorted_in, DenseRows<false>{});
    return hipGetLastError();
}

hipError_t launch_rows_update_decay(const RowsSegs &segs, int sorted_in, const int32_t *counters, float lr, float wd, float eps,
                                    hipStream_t st)
{
    int64_t threads = 0;
    for (int k = 0; k < segs.n_segs; ++k) {
        if (!segs.s[k].vec || !segs.s[k].steps) return hipErrorInvalidValue;
        threads = std::max<int64_t>(threads, (int64_t)segs.s[k].n << segs.s[k].lane_shift);
    }
    if (threads <= 0) return hipSuccess;
    hipLaunchKernelGGL(rows_update_decay_kernel, dim3((unsigned)((threads + 255) / 256), segs.n_segs), dim3(256), 0, st, segs, sorted_in,
                       counters, lr, wd, eps);
    return hipGetLastError();
}

hipError_t launch_rows_catch_up(const RowsCatchSeg *segs, int n_segs, const int32_t *counters, float lr, float wd, float eps,
                                hipStream_t st)
{
    if (n_segs < 0 || n_segs > ROWS_MAX_SEGS || !counters) return hipErrorInvalidValue;
    RowsCatchSegs a;
    std::memset(&a, 0, sizeof(a));
    for (int k = 0; k < n_segs; ++k) {
        if (segs[k].n <= 0) continue;
        a.s[a.n_segs] = segs[k];
        a.wave0[a.n_segs + 1] = a.wave0[a.n_segs] + (segs[k].n + ROWS_CATCH - 1) / ROWS_CATCH;
        ++a.n_segs;
    }
    const int64_t waves = a.wave0[a.n_segs];
    if (waves <= 0) return hipSuccess;
    hipLaunchKernelGGL(rows_catch_up_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, a, counters, lr, wd, eps);
    return hipGetLastError();
}

}  // namespace okge
