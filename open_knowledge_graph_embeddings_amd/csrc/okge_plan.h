// The host-side planner of the tile kernels' entry points (okge_api_*.hip): plain integer arithmetic on
// (B, N, d, the device's CU count, the five OKGE_* overrides), no HIP header, no global state -- it compiles with any
// C++17 compiler and tests/test_launch_plan.py drives it on the CPU (tests/plan_driver.cpp).  Three kinds of answer:
//   Shape                          the padded problem (make_shape)
//   SweepPlan, TrainPlan, Ranges   how a call is cut into launches (plan_sweep, plan_train, plan_ranges, plan_topk)
//   *Layout                        where each region of a call's workspace starts (one Arena each)
// No tile-kernel entry point (nor okge_adagrad_rows) computes a launch shape or a workspace offset outside this file.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "okge_consts.h"

#pragma GCC visibility push(hidden)   // inline functions of namespace okge, but none of them an export of the library
namespace okge {

constexpr size_t PLANE_CELL_BYTES = 16;   // sizeof(v8bf): one cell of a bf16 plane    } okge_core.hip asserts both against
constexpr size_t TOPK_REC_BYTES = 8;      // sizeof(TopkRec): (score, column)          } the device-side types

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Bump allocator of a workspace layout: every region starts on a 256-byte boundary
struct Arena {
    size_t off;
    explicit Arena(size_t start = 0) : off(align_up(start, 256)) {}
    size_t take(size_t bytes)
    {
        const size_t at = off;
        off += align_up(bytes, 256);
        return at;
    }
    size_t total() const { return off; }
};

// ---- the padded problem ---------------------------------------------------------------------------------------------------
struct Shape {
    int B, N, d, Bpad, KB, D16, LDK, ldq, tiles;
};

inline bool make_shape(int B, int N, int d, Shape &s)
{
    if (B <= 0 || N <= 0 || d <= 0) return false;
    s.B = B; s.N = N; s.d = d;
    s.Bpad = (B + BC - 1) / BC * BC;
    // slot size padded to a width the tile kernels are instantiated for (zero columns are free of error,
    // not of time: d in (128, 208] runs as 208, etc.)
    const int kb = (d + 15) / 16;
    s.KB = kb <= 4 ? 4 : kb <= 8 ? 8 : kb <= 13 ? 13 : kb <= 16 ? 16 : 32;
    s.D16 = 16 * s.KB;
    s.LDK = lds_ld(s.D16);
    s.ldq = s.D16;
    s.tiles = (N + NT - 1) / NT;
    return true;
}

// ---- the environment overrides --------------------------------------------------------------------------------------------
struct Knob {
    bool set = false;
    int  v = 0;
    int  value_or(int dflt) const { return set ? v : dflt; }
};
struct Knobs {
    Knob tail_split;   // OKGE_TAIL_SPLIT   0: never launch the closing round apart           (default 1)
    Knob gt_mbytes;    // OKGE_GT_MBYTES    MiB of G^T one candidate range may take           (default 1024)
    Knob b_split;      // OKGE_B_SPLIT      batch split of the train launch; set and nonzero also turns stream-K off (default: cost model)
    Knob streamk;      // OKGE_STREAMK      0: slot sizes above 256 train on the plain grid   (default 1)
    Knob dq_split;     // OKGE_DQ_SPLIT     candidate ranges of the dQ kernel                 (default: CUs / batch blocks)
};

inline Knob read_knob(const char *name)
{
    const char *v = std::getenv(name);
    Knob k;
    if (v && *v) { k.set = true; k.v = std::atoi(v); }
    return k;
}
// read per call: a process may change the environment between calls (the tests do)
inline Knobs read_knobs()
{
    Knobs k;
    k.tail_split = read_knob("OKGE_TAIL_SPLIT");
    k.gt_mbytes = read_knob("OKGE_GT_MBYTES");
    k.b_split = read_knob("OKGE_B_SPLIT");
    k.streamk = read_knob("OKGE_STREAMK");
    k.dq_split = read_knob("OKGE_DQ_SPLIT");
    return k;
}

// ---- launch plans ---------------------------------------------------------------------------------------------------------
// workgroups of a stream-K launch (slot sizes above 256): one per CU, (tile, 32-row chunk) units in equal runs
inline int streamk_wgs(int cus, int tiles, int chunks) { return (int)std::min<int64_t>(std::min(cus, 511), (int64_t)tiles * chunks); }

// Tail split of a launch of `tiles` equal tiles, one workgroup per CU (slot sizes up to 256): the `tail` tiles left over after
// whole rounds would cost a whole round's time; launched apart with the rows split `split` ways they cost 1 / split of it.
// Worth it when the rows per workgroup drop by at least two 64-row blocks.  (cfg4 shard: 4883 tiles = 19 rounds + 19 tiles.)
struct TailSplit { int tiles, split, b_per_block; };
inline TailSplit tail_split(int tiles, int Bpad, int slots, const Knobs &k)
{
    TailSplit t = {0, 0, Bpad};
    const int bblks = Bpad / BC, tail = tiles % slots;
    if (tiles <= slots || tail == 0 || k.tail_split.value_or(1) == 0) return t;
    const int c = std::min(slots / tail, bblks);
    if (c < 2) return t;
    const int per = (bblks + c - 1) / c;
    if (bblks - per < 2) return t;
    t.tiles = tail;
    t.b_per_block = per * BC;
    t.split = (Bpad + t.b_per_block - 1) / t.b_per_block;
    return t;
}

// One score / stats / count / top-k sweep of `tiles` 64-candidate tiles over all Bpad rows.  Slot sizes up to 256: main_tiles
// as (tile) workgroups, then, if tail_split > 1, the tail_tiles of the closing round as (tile, row split) workgroups of
// tail_b_per_block rows (rows are independent).  Above: sk_wgs > 0, the register-tile kernel in a stream-K launch.
struct SweepPlan {
    int tiles, main_tiles, tail_tiles, tail_split, tail_b_per_block, sk_wgs;
};
inline SweepPlan plan_sweep(const Shape &s, int tiles, int cus, const Knobs &k)
{
    SweepPlan p = {tiles, tiles, 0, 0, s.Bpad, 0};
    if (s.KB > 16) {
        p.sk_wgs = streamk_wgs(cus, tiles, (s.B + 31) / 32);
        return p;
    }
    const TailSplit ts = tail_split(tiles, s.Bpad, cus, k);
    if (ts.split > 1) { p.main_tiles = tiles - ts.tiles; p.tail_tiles = ts.tiles; p.tail_split = ts.split; p.tail_b_per_block = ts.b_per_block; }
    return p;
}

// Training (and the KL loss' row log-sum-exp, and top-k) sweeps the candidates in RANGES of range_n (a multiple of 64) so that
// the one (B, N)-shaped intermediate, G^T, and everything sized like it (masked rows Cm, KL statistics) is O(B x range_n):
// 41 GB -> 1 GB at |E| = 2.5 M, B = 4096.  A range is one tile-kernel launch + one dq launch (slabs accumulate).
struct Ranges {
    int range_tiles, n_ranges, range_n;
};
inline Ranges cut_ranges(int tiles, int range_tiles)
{
    Ranges r;
    r.range_tiles = range_tiles;
    r.n_ranges = (tiles + range_tiles - 1) / range_tiles;
    r.range_n = range_tiles * NT;
    return r;
}
// candidate ranges of the train step: G^T of one range stays under OKGE_GT_MBYTES (default 1024 MiB)
inline Ranges plan_ranges(const Shape &s, int cus, const Knobs &k)
{
    const int64_t budget = (int64_t)std::max(1, k.gt_mbytes.value_or(1024)) << 20;
    int64_t rt = budget / ((int64_t)s.Bpad * NT * (int64_t)sizeof(float));     // 64-candidate tiles per range
    rt = std::max<int64_t>(1, std::min<int64_t>(rt, s.tiles));
    const int n = (s.tiles + (int)rt - 1) / (int)rt;
    // slot sizes up to 256 run one workgroup per CU and tile: ranges of whole rounds (a multiple of the CU count: 256
    // tiles on an MI355X), so that only the LAST range ends in a partial round -- the one the tail split shortens
    if (n > 1 && s.KB <= 16 && rt >= cus) return cut_ranges(s.tiles, (int)(rt / cus * cus));
    return cut_ranges(s.tiles, (s.tiles + n - 1) / n);                  // even out the ranges
}

struct TrainPlan : Ranges {
    int ldg;                                     // leading dimension of G^T: the candidates of one range
    int b_split, b_per_block;                    // plain grid: (tiles, b_split) workgroups of b_per_block rows
    int sk_wgs, sk_chunks;                       // > 0: the train tile kernel is launched stream-K shaped over sk_wgs workgroups (okge_train64k.hip)
    // > 0: the LAST `tail_tiles` candidate tiles of the call (what is left over after whole rounds of one workgroup per CU)
    // are launched apart with the batch rows split over tail_split workgroups each, so the closing round is short
    int tail_tiles, tail_split, tail_b_per_block;
    int nsplit;                                  // dQ kernel: candidate ranges per batch block
    // what the launches write, counted once: the layout reserves from these and train_core launches from these
    int n_loss_partials;                         // doubles the tile launches leave for the loss reduction
    int dc_slabs, dc_slab_rows;                  // partial candidate-gradient slabs ([dc_slab_rows][D16] floats each); 0: dC_slab is not used
};

inline TrainPlan plan_train(const Shape &s, int cus, const Knobs &k)
{
    TrainPlan p;
    static_cast<Ranges &>(p) = plan_ranges(s, cus, k);
    p.ldg = p.range_tiles * NT;
    const int bblks = s.Bpad / BC;
    // fused train kernel: one 8-wave workgroup per CU on 64-candidate tiles (slot sizes above 256: fused_tile64k_kernel,
    // candidate tile in registers)
    const int slots = cus;
    // fill the CUs: if there are few candidate tiles, split the batch rows across blockIdx.y.  Cost of a split into c:
    // (rounds of workgroups over the slots) x (row blocks per workgroup + 1) -- the "+ 1" is a workgroup's fixed cost, the
    // candidate gather and the gradient write-back, about one 64-row block (profiles/round2_ablation.md §1) -- plus the c
    // partial-gradient slabs dc_reduce adds up (an eighth of a block each).  Measured at cfg3 on the retired 32-candidate cut
    // (313 tiles of 32, d = 512):
    // c = 1 / 2 / 3 / 4 / 8 -> 0.299 / 0.288 / 0.294 / 0.303 / 0.364 ms per step; the model orders them 18 / 15 / 16 / 15 / 20.
    int bs = 1;
    {
        long best = -1;
        for (int c = 1; c <= bblks; ++c) {
            const long rounds = ((long)s.tiles * c + slots - 1) / slots, per = (bblks + c - 1) / c;
            const long cost = 8 * rounds * (per + 1) + c;
            if (best < 0 || cost < best) { best = cost; bs = c; }
        }
    }
    bs = std::max(1, k.b_split.value_or(bs));
    bs = std::min(bs, bblks);
    p.b_per_block = (bblks + bs - 1) / bs * BC;
    p.b_split = (s.Bpad + p.b_per_block - 1) / p.b_per_block;
    if (p.n_ranges > 1) { p.b_split = 1; p.b_per_block = s.Bpad; }   // many tiles: no batch split
    // slot sizes above 256 (fused_tile64k_kernel), one launch: (tile, 32-row chunk) units in equal runs over one workgroup
    // per CU instead of a (tiles, batch splits) grid -- see the kernel's header for the measurements behind it
    p.sk_wgs = p.sk_chunks = 0;
    if (s.KB == 32 && p.n_ranges == 1 && k.streamk.value_or(1) != 0 && k.b_split.value_or(0) == 0) {
        p.sk_chunks = (s.B + 31) / 32;
        p.sk_wgs = streamk_wgs(cus, s.tiles, p.sk_chunks);
        p.b_split = 1;
        p.b_per_block = s.Bpad;
    }
    // tail split (slot sizes up to 256, more tiles than CUs): equal tiles in rounds of one per CU leave a closing round with
    // `tail` < 256 workgroups that still takes a whole round's time (cfg4 shard: 4883 tiles = 19 rounds + 19 tiles -> 20 rounds,
    // 4.6 % of the kernel idle).  The tail tiles are launched apart with the rows split floor(256 / tail) ways; their partial
    // candidate gradients go through the batch-split slabs + dc_reduce.  Worth it when the rows per workgroup drop by >= 2 blocks.
    p.tail_tiles = p.tail_split = 0;
    p.tail_b_per_block = s.Bpad;
    if (s.KB <= 16 && p.b_split == 1) {
        const TailSplit ts = tail_split(s.tiles - (p.n_ranges - 1) * p.range_tiles, s.Bpad, slots, k);
        if (ts.split > 1) { p.tail_tiles = ts.tiles; p.tail_split = ts.split; p.tail_b_per_block = ts.b_per_block; }
    }
    // dQ kernel: (batch block, candidate range) workgroups, 8 waves, one per CU
    int ns = std::max(1, cus / bblks);
    if (ns >= 8) ns = ns / 8 * 8;   // workgroups of one candidate range then share an XCD (blockIdx % 8)
    ns = k.dq_split.value_or(ns);
    p.nsplit = std::max(1, std::min(ns, p.range_tiles));
    // (tail split: the tail launch's partials of row split y > 0 follow the per-tile ones -- index y * tail + x from the tail's
    //  first tile is contiguous with them)
    p.n_loss_partials = p.sk_wgs > 0 ? p.sk_wgs : s.tiles * p.b_split + p.tail_tiles * std::max(0, p.tail_split - 1);
    // stream-K: two slabs of one tile per workgroup (dc_reduce_streamk); batch split (always a single range): one slab of all
    // tiles per split; tail split: one slab of the tail tiles per row split
    p.dc_slabs = p.dc_slab_rows = 0;
    if (p.sk_wgs > 0) { p.dc_slabs = 2 * p.sk_wgs; p.dc_slab_rows = NT; }
    else if (p.b_split > 1) { p.dc_slabs = p.b_split; p.dc_slab_rows = s.tiles * NT; }
    else if (p.tail_split > 1) { p.dc_slabs = p.tail_split; p.dc_slab_rows = p.tail_tiles * NT; }
    return p;
}

// ---- workspace layouts ----------------------------------------------------------------------------------------------------
// the query block every layout opens with: folded queries [Bpad][ldq]
inline size_t take_query_block(Arena &ar, const Shape &s) { return ar.take((size_t)s.Bpad * s.ldq * sizeof(float)); }

struct ScoreLayout { size_t off_Q, total; };
inline ScoreLayout score_layout(const Shape &s)
{
    Arena ar;
    ScoreLayout l;
    l.off_Q = take_query_block(ar, s);
    l.total = ar.total();
    return l;
}

struct LseLayout {
    size_t off_Q, off_tptr, off_stats, off_lse, off_ysum, off_run;
    size_t score_bytes, lse_bytes;
};
struct TrainLayout : LseLayout {
    size_t off_loss, off_GT, off_Cm, off_slab, off_dcs, off_Qp;
    size_t loss_bytes, dcs_bytes;       // capacity of the two regions the plan's derived counts must fit
    size_t total;
};

inline void lay_out_lse(Arena &ar, const Shape &s, const Ranges &r, LseLayout &l)
{
    // [score-only part] the query block
    l.off_Q = take_query_block(ar, s);
    l.score_bytes = ar.total();
    // [row log-sum-exp part] per-range (max, sum-exp) tile statistics + the running per-row state
    // (the tile offsets here and the loss partials below keep room for 32-candidate tiles, so that okge_train_workspace_bytes
    //  answers as it did before that cut was retired)
    l.off_tptr = ar.take((size_t)(2 * s.tiles + 1) * sizeof(int32_t));
    l.off_stats = ar.take((size_t)4 * r.range_tiles * s.Bpad * 2 * sizeof(float));   // <= 4 per tile
    l.off_lse = ar.take((size_t)s.Bpad * sizeof(float));
    l.off_ysum = ar.take((size_t)s.Bpad * sizeof(float));
    l.off_run = ar.take((size_t)s.Bpad * 2 * sizeof(float));
    l.lse_bytes = ar.total();
}

inline LseLayout lse_layout(const Shape &s, const Ranges &r)
{
    Arena ar;
    LseLayout l;
    lay_out_lse(ar, s, r, l);
    return l;
}

inline TrainLayout train_layout(const Shape &s, const TrainPlan &p)
{
    Arena ar;
    TrainLayout l;
    lay_out_lse(ar, s, p, l);
    // [training part]  (loss partials: room as for 32-candidate tiles, see above -- at least twice what the plan writes)
    l.loss_bytes = (size_t)std::max(2 * s.tiles * p.b_split + p.tail_tiles * p.tail_split, p.sk_wgs) * sizeof(double);
    l.off_loss = ar.take(l.loss_bytes);
    l.off_GT = ar.take((size_t)s.Bpad * p.ldg * sizeof(float));
    // masked candidate rows of a range: three bf16 planes (6 bytes per element) up to slot size 208, fp32 rows above
    l.off_Cm = ar.take(s.KB <= 13 ? (size_t)p.range_tiles * plane_cells_per_tile(s.D16) * PLANE_CELL_BYTES
                                  : (size_t)p.range_tiles * NT * s.D16 * sizeof(float));
    l.off_slab = ar.take((size_t)p.nsplit * s.Bpad * s.ldq * sizeof(float));
    l.dcs_bytes = (size_t)p.dc_slabs * p.dc_slab_rows * s.D16 * sizeof(float);
    l.off_dcs = ar.take(l.dcs_bytes);
    // the folded queries once more as three bf16 planes, for the tile kernel's gradient product (okge_tile_grad_split.h)
    l.off_Qp = ar.take(tile_grad_split(s.KB) ? (size_t)s.Bpad * s.D16 * 6 : 0);
    l.total = ar.total();
    return l;
}

// OKGE_TRAIN_ROW_GRADS: the occurrence rows of the batch behind the step's own scratch -- EV = [candidate rows | prefix entity
// rows], RV = relation rows, then the positions that stand in for ids
struct RowGradsLayout { size_t off_EV, off_RV, off_ids, total; };
inline RowGradsLayout row_grads_layout(const Shape &s, size_t train_total)
{
    Arena ar(train_total);
    RowGradsLayout l;
    l.off_EV = ar.take((size_t)(s.N + s.B) * s.d * sizeof(float));
    l.off_RV = ar.take((size_t)s.B * s.d * sizeof(float));
    l.off_ids = ar.take((size_t)2 * s.B * sizeof(int32_t));
    l.total = ar.total();
    return l;
}

// Top-k link prediction.  The sweep runs per candidate range; a range leaves [tiles of the range][Bpad][k] records and one merge
// launch folds them into the running (B, k) list, which IS the caller's output.  Default range: the records (plus, above slot
// size 256, the range's score block) stay under TOPK_PARTIAL_CAP; whole rounds of one tile per CU when a range is that long, as
// in training.
constexpr size_t TOPK_PARTIAL_CAP = (size_t)256 << 20;
struct TopkPlan : Ranges { size_t off_Q, off_part, off_X, total; };
inline bool plan_topk(const Shape &s, int k, int range_n, int cus, TopkPlan &p)
{
    if (k < 1 || k > 64 || range_n < 0 || s.d > 512) return false;
    const bool wide = s.KB > 16;
    const size_t per_tile = (size_t)s.Bpad * ((size_t)k * TOPK_REC_BYTES + (wide ? NT * sizeof(float) : 0));
    int64_t rt;
    if (range_n > 0) {
        rt = std::max(1, range_n / NT);
    } else {
        rt = std::max<int64_t>(1, (int64_t)(TOPK_PARTIAL_CAP / per_tile));
        if (!wide && rt >= cus) rt = rt / cus * cus;
    }
    static_cast<Ranges &>(p) = cut_ranges(s.tiles, (int)std::min<int64_t>(rt, s.tiles));
    Arena ar;
    p.off_Q = take_query_block(ar, s);                           // (okge_topk_prefixes)
    p.off_part = ar.take((size_t)p.range_tiles * s.Bpad * k * TOPK_REC_BYTES);
    p.off_X = ar.take(wide ? (size_t)s.Bpad * p.range_n * sizeof(float) : 0);
    p.total = ar.total();
    return true;
}

// Fused evaluation: the query block, then the point scores, the sorted batch and the rank counters
constexpr size_t EVAL_SLAB_MAX = (size_t)256 << 20;      // per-tile count slabs up to 256 MB; beyond that: atomics
struct EvalLayout { size_t off_Q, off_true, off_filt, off_rps, off_gshift, off_grow, off_counts, total; bool slab; };
inline bool eval_layout(const Shape &s, int64_t n_groups, int64_t n_filter, EvalLayout &e)
{
    if (n_groups < 0 || n_filter < 0) return false;
    const size_t groups = (size_t)std::max<int64_t>(n_groups, 1);
    Arena ar;
    e.off_Q = take_query_block(ar, s);
    e.off_true = ar.take(groups * sizeof(float));
    e.off_filt = ar.take((size_t)std::max<int64_t>(n_filter, 1) * sizeof(float));
    e.off_rps = ar.take((size_t)(s.Bpad + 1) * sizeof(int64_t));       // row_ptr of the batch sorted by group count
    e.off_gshift = ar.take((size_t)s.Bpad * sizeof(int64_t));          // original -> sorted group index, per row
    e.off_grow = ar.take(groups * sizeof(int32_t));                    // row of every group
    const size_t slab_bytes = (size_t)s.tiles * groups * sizeof(uint32_t);
    e.slab = slab_bytes <= EVAL_SLAB_MAX;
    e.off_counts = ar.take(e.slab ? slab_bytes : groups * 2 * sizeof(int32_t));
    e.total = ar.total();
    return true;
}

// The validation loss of an evaluation batch (okge_evaluate_*_loss) keeps its scratch BEHIND the call's own workspace, so
// that eval_layout / score_layout answer as they do without a loss.  Fused: one float2 per (tile, row) from the sweep, the
// label term (sum and number of the positives' scores) per row from the points launch, the rows' losses.  Materialising:
// the rows' losses only.
struct EvalLossLayout { size_t off_part, off_pos, off_npos, off_rows, total; };
inline EvalLossLayout eval_loss_layout(const Shape &s, size_t eval_total)
{
    Arena ar(eval_total);
    EvalLossLayout l;
    l.off_part = ar.take((size_t)s.tiles * s.Bpad * 2 * sizeof(float));
    l.off_pos = ar.take((size_t)s.Bpad * sizeof(double));
    l.off_npos = ar.take((size_t)s.Bpad * sizeof(int32_t));
    l.off_rows = ar.take((size_t)s.Bpad * sizeof(double));
    l.total = ar.total();
    return l;
}
struct BlockLossLayout { size_t off_rows, total; };
inline BlockLossLayout block_loss_layout(int B, size_t score_total)
{
    Arena ar(score_total);
    BlockLossLayout l;
    l.off_rows = ar.take((size_t)std::max(B, 1) * sizeof(double));
    l.total = ar.total();
    return l;
}

// okge_adagrad_rows: the two sort-key buffers of a tensor of n > 0 occurrence rows
struct RowsKeys { size_t off[2]; };
inline RowsKeys take_rows_keys(Arena &ar, int64_t n)
{
    RowsKeys k;
    k.off[0] = ar.take((size_t)n * sizeof(uint64_t));
    k.off[1] = ar.take((size_t)n * sizeof(uint64_t));
    return k;
}

// ---- the wide path: slot sizes 513 .. 4096 (okge_wide.hip) ------------------------------------------
// Unfused: wide_tile_kernel contracts over d in LDS-staged chunks and leaves G = dLoss/dScore / normalizer of one candidate
// range in the workspace; the two backward products run on gemm_f32_kernel (okge_gemm.hip), where d is a free dimension.
// Nothing above this line changes for it: a wide call has its own shape, plan and layouts.
constexpr int WIDE_MAX_D = 4096;                 // slot sizes 513 .. WIDE_MAX_D take the wide path
constexpr int WIDE_TM = 128, WIDE_TN = 128;      // output tile of wide_tile_kernel: batch rows x candidates per workgroup
constexpr int WIDE_KC = 16;                      // columns of d per LDS-staged chunk (and the padding unit of ldq)
constexpr int WIDE_GEMM_TILE = 64, WIDE_GEMM_K = 16;   // gemm_f32_kernel's output tile and K chunk (okge_gemm.hip)
inline bool is_wide(int d) { return d > 512 && d <= WIDE_MAX_D; }

struct WideShape {
    int B, N, d, Bpad, ldq, tiles, row_blocks;
};
inline bool make_wide_shape(int B, int N, int d, WideShape &s)
{
    if (B <= 0 || N <= 0 || !is_wide(d)) return false;
    s.B = B; s.N = N; s.d = d;
    s.row_blocks = (B + WIDE_TM - 1) / WIDE_TM;
    s.Bpad = s.row_blocks * WIDE_TM;
    s.ldq = (d + WIDE_KC - 1) / WIDE_KC * WIDE_KC;
    s.tiles = (N + WIDE_TN - 1) / WIDE_TN;
    return true;
}

// Candidate ranges of whole 128-candidate tiles: G [Bpad][range_n], the gathered masked rows Cm [range_n][ldq] and their
// gradient dC [range_n][ldq] of ONE range stay under OKGE_GT_MBYTES (a range is never shorter than one tile).  The dQ product of
// a range is split over K = the range's candidates into dq_splits slabs of dq_k_per candidates, added in split order.
struct WidePlan : Ranges {
    int    ldg;                  // leading dimension of G: the candidates of one range
    int    dq_splits, dq_k_per;
    int    n_loss_partials;      // one double per (candidate tile, row block)
    size_t tile_bytes;           // G + Cm + dC of one tile of a range
};
inline WidePlan plan_wide(const WideShape &s, const Knobs &k)
{
    WidePlan p;
    const int64_t budget = (int64_t)std::max(1, k.gt_mbytes.value_or(1024)) << 20;
    p.tile_bytes = (size_t)WIDE_TN * ((size_t)s.Bpad + 2 * (size_t)s.ldq) * sizeof(float);
    int64_t rt = budget / (int64_t)p.tile_bytes;
    rt = std::max<int64_t>(1, std::min<int64_t>(rt, s.tiles));
    p.n_ranges = (s.tiles + (int)rt - 1) / (int)rt;
    p.range_tiles = (s.tiles + p.n_ranges - 1) / p.n_ranges;      // even out the ranges
    p.n_ranges = (s.tiles + p.range_tiles - 1) / p.range_tiles;
    p.range_n = p.range_tiles * WIDE_TN;
    p.ldg = p.range_n;
    // dQ = G . Cm has few output tiles and a long contraction: split it, at most 1024 workgroups and 64 slabs
    const int out_tiles = ((s.B + WIDE_GEMM_TILE - 1) / WIDE_GEMM_TILE) * ((s.d + WIDE_GEMM_TILE - 1) / WIDE_GEMM_TILE);
    const int kn = std::min(p.range_n, s.N);
    int splits = std::max(1, std::min(64, std::min(1024 / out_tiles, (kn + 4 * WIDE_GEMM_K - 1) / (4 * WIDE_GEMM_K))));
    p.dq_k_per = ((kn + splits - 1) / splits + WIDE_GEMM_K - 1) / WIDE_GEMM_K * WIDE_GEMM_K;
    p.dq_splits = (kn + p.dq_k_per - 1) / p.dq_k_per;
    p.n_loss_partials = s.tiles * s.row_blocks;
    return p;
}

struct WideScoreLayout { size_t off_Q, total; };
inline WideScoreLayout wide_score_layout(const WideShape &s)
{
    Arena ar;
    WideScoreLayout l;
    l.off_Q = ar.take((size_t)s.Bpad * s.ldq * sizeof(float));
    l.total = ar.total();
    return l;
}

struct WideTrainLayout {
    size_t off_Q, off_tptr, off_stats, off_lse, off_ysum, off_run;      // the score / row log-sum-exp part
    size_t score_bytes, lse_bytes;
    size_t off_loss, off_G, off_Cm, off_dC, off_dQ, off_slab;           // the training part
    size_t total;
};
inline WideTrainLayout wide_train_layout(const WideShape &s, const WidePlan &p)
{
    Arena ar;
    WideTrainLayout l;
    l.off_Q = ar.take((size_t)s.Bpad * s.ldq * sizeof(float));
    l.score_bytes = ar.total();
    l.off_tptr = ar.take((size_t)(s.tiles + 1) * sizeof(int32_t));
    l.off_stats = ar.take((size_t)p.range_tiles * s.Bpad * 2 * sizeof(float));
    l.off_lse = ar.take((size_t)s.Bpad * sizeof(float));
    l.off_ysum = ar.take((size_t)s.Bpad * sizeof(float));
    l.off_run = ar.take((size_t)s.Bpad * 2 * sizeof(float));
    l.lse_bytes = ar.total();
    l.off_loss = ar.take((size_t)p.n_loss_partials * sizeof(double));
    l.off_G = ar.take((size_t)s.Bpad * p.ldg * sizeof(float));
    l.off_Cm = ar.take((size_t)p.range_n * s.ldq * sizeof(float));
    l.off_dC = ar.take((size_t)p.range_n * s.ldq * sizeof(float));
    l.off_dQ = ar.take((size_t)s.Bpad * s.ldq * sizeof(float));
    l.off_slab = ar.take((size_t)p.dq_splits * s.Bpad * s.ldq * sizeof(float));
    l.total = ar.total();
    return l;
}

// ---- the N3 regulariser (okge_n3.hip) ---------------------------------------------------------------
// Elementwise over the N candidate rows and the 2 B prefix rows (B entity rows, then B relation rows), in items of one
// 8-column octet (the unit of a dropout mask draw).  A workgroup takes whole rows, N3_ITEMS items of them (one row above
// 8 * N3_ITEMS columns), and leaves one double partial of the value: the grid, and with it the order of the value's sum,
// depends on (B, N, d) alone.  (Four items per thread: measured against one per thread at the S-FB shape, d = 2048 -- 0.12
// against 0.16 ms for the sweep -- and no different at d = 200.)
constexpr int N3_THREADS = 256, N3_ITEMS = 1024;
struct N3Plan {
    int    n_oct, rows_per_wg, cand_wgs, prefix_wgs;
    size_t total;                // the workspace: one double per workgroup
};
inline bool plan_n3(int B, int N, int d, N3Plan &p)
{
    if (B <= 0 || N <= 0 || d <= 0 || d > WIDE_MAX_D) return false;
    p.n_oct = (d + 7) / 8;
    p.rows_per_wg = std::max(1, N3_ITEMS / p.n_oct);
    p.cand_wgs = (N + p.rows_per_wg - 1) / p.rows_per_wg;
    p.prefix_wgs = (2 * B + p.rows_per_wg - 1) / p.rows_per_wg;
    Arena ar;
    ar.take((size_t)(p.cand_wgs + p.prefix_wgs) * sizeof(double));
    p.total = ar.total();
    return true;
}

// ---- the lookup embedder variants' encode (okge_lookup_encode.hip) ------------------------------------
// One pass = the encode calls of a batch; their rows are numbered entity calls first, then relation calls.  Batch-norm column
// sums are taken over chunks of LOOKUP_BN_CHUNK rows of one call and added in chunk order; the projection's weight gradients
// over at most LOOKUP_MAX_SPLITS slabs of rows, added in slab order.  Eval mode keeps the forward's regions only.
constexpr int LOOKUP_MAX_CALLS = 8, LOOKUP_BN_CHUNK = 128, LOOKUP_MAX_SPLITS = 16, LOOKUP_MAX_D = 512;
struct LookupLayout {
    size_t off_X;        // [rows][d]  gathered rows behind the input dropout
    size_t off_saved;    // [LOOKUP_MAX_CALLS][4 d]  per call, at 2 d: the call's d weight, d bias (the layout enc_bn_grad_kernel reads)
    size_t off_stat;     // [LOOKUP_MAX_CALLS][2 d] doubles: per call the batch mean and rstd
    size_t off_part;     // [max_chunks][2 d] doubles: the chunks' column sums
    size_t off_norm;     // [rows] doubles: row norms (normalize='norm')
    size_t off_Wt;       // [2][d][d]  the two projection weights, transposed
    size_t off_P;        // [entity rows][d]  projected rows in front of the normalisation
    size_t off_G1;       // training: [rows][d]  gradient behind the normalisation / activation backward
    size_t off_G2;       // training: [entity rows][d]  gradient behind the projection backward
    size_t off_slab;     // training: [2][LOOKUP_MAX_SPLITS][d][d]  partial weight gradients
    size_t off_Xbn;      // training: [entity rows][d]  the batch-normed rows the projection read
    size_t total;
    int    max_chunks;   // chunks of a pass at most: every call may end in a partial chunk
};
inline bool lookup_layout(int64_t ent_rows, int64_t rel_rows, int d, bool training, LookupLayout &l)
{
    const int64_t rows = ent_rows + rel_rows;
    if (ent_rows < 0 || rel_rows < 0 || rows <= 0 || d <= 0 || d > LOOKUP_MAX_D || rows * d > INT32_MAX) return false;
    Arena ar;
    l.max_chunks = (int)((rows + LOOKUP_BN_CHUNK - 1) / LOOKUP_BN_CHUNK) + LOOKUP_MAX_CALLS;
    l.off_X = ar.take((size_t)rows * d * sizeof(float));
    l.off_saved = ar.take((size_t)LOOKUP_MAX_CALLS * 4 * d * sizeof(float));
    l.off_stat = ar.take((size_t)LOOKUP_MAX_CALLS * 2 * d * sizeof(double));
    l.off_part = ar.take((size_t)l.max_chunks * 2 * d * sizeof(double));
    l.off_norm = ar.take((size_t)rows * sizeof(double));
    l.off_Wt = ar.take((size_t)2 * d * d * sizeof(float));
    l.off_P = ar.take((size_t)ent_rows * d * sizeof(float));
    l.off_G1 = l.off_G2 = l.off_slab = l.off_Xbn = ar.total();
    if (training) {
        l.off_G1 = ar.take((size_t)rows * d * sizeof(float));
        l.off_G2 = ar.take((size_t)ent_rows * d * sizeof(float));
        l.off_slab = ar.take((size_t)2 * LOOKUP_MAX_SPLITS * d * d * sizeof(float));
        l.off_Xbn = ar.take((size_t)ent_rows * d * sizeof(float));
    }
    l.total = ar.total();
    return true;
}

}  // namespace okge
#pragma GCC visibility pop
