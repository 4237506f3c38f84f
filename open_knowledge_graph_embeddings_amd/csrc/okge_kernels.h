// Kernel argument blocks and launcher prototypes shared by the .hip translation units.
#pragma once
#include <string>
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include "okge_consts.h"      // NT, BC, plane_cells_per_tile, tile_grad_split, lds_ld
#include "okge_device.h"
#include "okge_topk.h"
#include "../../include/okge.h"

namespace okge {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-DEVICE setting: launch_with_lds keeps one of these per kernel
// and opts the kernel in once per device (and again if a larger size is asked for), keyed by
// hipGetDevice() -- one process per GPU is the normal deployment, but a process driving two devices must work too.
struct LdsOptIn {
    std::atomic<size_t> bytes[64];
    LdsOptIn() { for (auto &b : bytes) b.store(0, std::memory_order_relaxed); }
};
inline hipError_t ensure_dynamic_lds(LdsOptIn &state, const void *kernel, size_t shmem)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    if (shmem <= state.bytes[dev].load(std::memory_order_acquire)) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);      // (idempotent: a race repeats it)
    if (e == hipSuccess) state.bytes[dev].store(shmem, std::memory_order_release);
    return e;
}
#ifdef __HIPCC__
// Launch of a kernel that may need more dynamic LDS than the default limit.  One instantiation, hence one opt-in state, per
// kernel.
template <auto Kernel, class Args>
inline hipError_t launch_with_lds(dim3 grid, dim3 block, size_t shmem, hipStream_t st, const Args &args)
{
    static LdsOptIn lds_opt_in;
    if (hipError_t e = ensure_dynamic_lds(lds_opt_in, reinterpret_cast<const void *>(Kernel), shmem); e != hipSuccess) return e;
    hipLaunchKernelGGL(Kernel, grid, block, shmem, st, args);
    return hipGetLastError();
}
#endif

constexpr int LDG = 68;            // leading dimension of the 64x64 G / X tile in LDS (4*odd)
constexpr int FUSED_THREADS = 512; // 8 waves, two per SIMD (fused_tile_kernel: score / stats / count sweep)
constexpr int POS_CACHE = 512;     // positives of one candidate tile cached in LDS (more spill to global reads)

enum { MODE_TRAIN_BCE = 0, MODE_SCORE = 1, MODE_STATS = 2, MODE_TRAIN_KL = 3, MODE_COUNT = 4, MODE_TOPK = 5,
       // MODE_COUNT that also leaves, in `stats`, one float2 per (tile, row): the row's validation-loss partial over the tile
       MODE_COUNT_BCE = 6, MODE_COUNT_KL = 7,
       // the training modes WITHOUT the candidate-gradient product dC = G^T . Q (OKGE_TRAIN_FREEZE_ENTITIES): score, loss and G
       // as MODE_TRAIN_*, no dC accumulators, no write-back.  Modes of their own, so the MODE_TRAIN_* instantiations are
       // the kernels they were, names included
       MODE_TRAIN_BCE_NODC = 8, MODE_TRAIN_KL_NODC = 9 };
__host__ __device__ constexpr bool mode_trains(int mode)
{
    return mode == MODE_TRAIN_BCE || mode == MODE_TRAIN_KL || mode == MODE_TRAIN_BCE_NODC || mode == MODE_TRAIN_KL_NODC;
}
__host__ __device__ constexpr bool mode_no_dc(int mode) { return mode == MODE_TRAIN_BCE_NODC || mode == MODE_TRAIN_KL_NODC; }
// the loss a training mode computes, as the mode that loss_element takes
__host__ __device__ constexpr int mode_loss(int mode) { return mode == MODE_TRAIN_BCE_NODC ? MODE_TRAIN_BCE : mode == MODE_TRAIN_KL_NODC ? MODE_TRAIN_KL : mode; }
__host__ __device__ constexpr bool mode_counts(int mode) { return mode == MODE_COUNT || mode == MODE_COUNT_BCE || mode == MODE_COUNT_KL; }
__host__ __device__ constexpr bool mode_count_loss(int mode) { return mode == MODE_COUNT_BCE || mode == MODE_COUNT_KL; }
enum { LOSS_BCE = 0, LOSS_KL = 1 };
enum { SC_COMPLEX = 0, SC_DISTMULT = 1, SC_BIAS_RELATION = 2, SC_BIAS_ENTITY = 3 };   // = enum okge_scorer
// the data-bias scorers (model.py:281-350): the folded query row is a copy of ONE masked row
__host__ __device__ constexpr bool sc_is_bias(int scorer) { return scorer == SC_BIAS_RELATION || scorer == SC_BIAS_ENTITY; }

struct FusedArgs {
    const float   *E;          // entity table (n_ent, d)
    const int32_t *cand_ids;   // nullptr => cand_first + position
    const float   *Q;          // folded queries [Bpad][ldq], zero padded to ldq >= D16
    const int32_t *pos_col, *pos_row;
    const int32_t *tile_ptr;   // [tiles + 1] offsets into pos_* per candidate tile
    const float   *row_lse, *row_ysum;   // KL
    float         *G;          // [Bpad][ldg]  dLoss/dX / normalizer, row-major, ldg = 64 * tiles
    float         *Cm;         // [64 * tiles][16*KB]  masked (dropped-out) candidate rows, for the dQ kernel (slot sizes above 208)
    float         *dE;
    float         *dC_slab;    // [gridDim.y][64 * tiles][16*KB] partial candidate gradients when the batch is split over blockIdx.y
    double        *loss_partial;
    float         *X;          // score mode
    float         *stats;      // stats mode: float2 [tiles][Bpad]; MODE_COUNT_BCE / _KL: the rows' loss partials, same layout
    // count mode (fused evaluation): per answer group of every row, how many of the tile's scores are greater than /
    // equal to the group's true score -> atomically added to rk_counts[group][2]
    const int64_t *rk_row_ptr; // [B + 1] groups of each row
    const float   *rk_true;    // [n_groups]
    int32_t       *rk_counts;  // [n_groups][2]   (atomics; used when the slab would be too large)
    uint32_t      *rk_slab;    // [tiles][n_groups] packed (#greater | #equal << 16) of every tile: plain coalesced stores
    int64_t        rk_ngroups;
    unsigned long long *stamps_dbg;   // diagnostic build (-DOKGE_STAMPS) only
    int64_t        ldx;
    DropDev        drop_c;
    int32_t        d, KB, LDK, cand_first, N, B, Bpad, ldq, ldg, nnz, b_per_block, loss_kind, x_vec_ok, grads_zero, cand_exclusive;
    float          y_pos, y_neg, inv_norm;
    int32_t        cand_col0;  // global column (candidate position) of local candidate 0: positives, dropout keys
    int64_t        n_table_rows;   // rows of the table `E` points to: candidate ids are checked against it (checked_row)
    int           *id_err;         // device word counting out-of-range ids
    int32_t        loss_only;  // forward + loss only: no G store, no dC product, no write-back
    int32_t        sk_tiles;   // fused_tile64k_kernel: > 0 = stream-K launch over this many candidate tiles (grid = workgroups)
    v8bf          *Cplanes;    // [tiles][plane_cells_per_tile]  slot sizes up to 208: the masked candidate rows as three bf16 planes, in place of Cm
    const v8bf    *Qplanes;    // [Bpad / 64][chunk image]  tile_grad_split(KB): Q as three bf16 planes (okge_tile_grad_split.h)
    // top-k mode (okge_topk.h): per (tile, row) the tile's best tk_k eligible candidates as (score, global column) records
    TopkRec       *tk_part;    // [tiles][Bpad][tk_k]
    const int64_t *tk_filt_ptr;   // [B + 1] CSR of each row's filtered GLOBAL columns (ascending), or nullptr
    const int32_t *tk_filt_col;
    int32_t        tk_k;
};

struct DqArgs {
    const float   *G;
    const float   *Cm;         // masked candidate rows written by the tile kernel: fp32 rows (dq8k_kernel) ...
    const v8bf    *Cplanes;    // ... or their three bf16 planes (dq8s_kernel); the other one is nullptr
    float         *slab;       // [nsplit][Bpad][ldq]
    int32_t        d, KB, LDK, N, Bpad, ldq, ldg, nsplit;
    int32_t        accumulate; // add to the slabs instead of overwriting them (candidate ranges after the first)
};

struct PrefixDev {
    const int32_t *po_rel, *po_obj, *sp_subj, *sp_rel;
    int32_t        n_po, n_sp;
    int32_t        ent_lo, ent_hi;   // global entity ids [ent_lo, ent_hi) live in the local table (row = id - ent_lo)
    int32_t        n_rel;            // rows of the relation table; whole_table: ent range IS the table (an id outside is an error,
    int32_t        whole_table;      // not another rank's row)
    int           *id_err;           // device word counting out-of-range ids
    DropDev        drop_po_ent, drop_po_rel, drop_sp_ent, drop_sp_rel;
};

size_t     fused_shmem_bytes(int LDK);
hipError_t launch_fused(int mode, const FusedArgs &a, int grid_x, int grid_y, hipStream_t st);
hipError_t launch_dq(const DqArgs &a, int grid_x, hipStream_t st);
hipError_t launch_dq8s(const DqArgs &a, int grid_x, hipStream_t st);   // slot sizes up to 208 (KB = 4, 8, 13): bf16 three-plane product
hipError_t launch_fused64(int mode, const FusedArgs &a, int grid_x, int grid_y, hipStream_t st);
hipError_t launch_fused64k(int mode, const FusedArgs &a, int grid_x, int grid_y, hipStream_t st);   // slot sizes above 256

// up to four float regions cleared by extra workgroups of encode_queries_kernel (OKGE_TRAIN_CLEAR_GRADS: dR, dE in front of
// and behind the candidates; the KL loss' per-row label mass before it is counted)
constexpr int CLEAR_REGIONS = 4;
struct ClearSpec { float *p[CLEAR_REGIONS]; int64_t n[CLEAR_REGIONS]; };
hipError_t launch_encode_queries(const float *E, const float *R, int d, int scorer, const PrefixDev &p, float *Q,
                                 int ldq, int Bpad, float *ent_rows, const int32_t *pos_col, int nnz, int32_t *tile_ptr,
                                 int tiles, int tile_w, int cand_col0, hipStream_t st, const ClearSpec *clear = nullptr,
                                 v8bf *q_planes = nullptr, int KB = 0);       // q_planes: Q also as three bf16 planes (okge_tile_grad_split.h)
// the same planes from a query block computed elsewhere: rows B .. Bpad - 1 are not read and come out as zero planes
hipError_t launch_query_planes(const float *Q, int ldq, int B, int Bpad, int d, int KB, v8bf *q_planes, hipStream_t st);
hipError_t launch_fold_queries(const float *R, int d, int scorer, const PrefixDev &p, const float *ent_rows, float *Q, int ldq,
                               int Bpad, hipStream_t st);
hipError_t launch_slab_reduce(const float *slab, int nsplit, int64_t n, float *out, const double *loss_partials,
                              int n_partials, double *loss_out, hipStream_t st);
hipError_t launch_prefix_backward(const float *E, const float *R, int d, int scorer, const PrefixDev &p,
                                  const float *slab, int nsplit, int Bpad, int ldq, const float *ent_rows, float *dE,
                                  float *dR, const double *loss_partials, int n_partials, double *loss_out,
                                  hipStream_t st, const int32_t *rel_order = nullptr, const int32_t *rel_seg_ptr = nullptr,
                                  int n_rel_seg = 0, const int32_t *ent_order = nullptr, const int32_t *ent_seg_ptr = nullptr,
                                  int n_ent_seg = 0, float *grad_rows = nullptr, int distinct = 0);
// the data-bias scorers' chain-rule launch (okge_bias.hip; called by launch_prefix_backward): d % 4 == 0 -> the float4 kernel
// (which also reduces the loss partials and may store rows to dr_rows / de_rows), otherwise the scalar kernel; neither table is
// read: the gradient of a copy needs no operand
hipError_t launch_bias_prefix_rows(int d, int scorer, const PrefixDev &p, const float *slab,
                                   int nsplit, int Bpad, int ldq, const float *ent_rows, float *dE, float *dR,
                                   const double *loss_partials, int n_partials, double *loss_out, float *dr_rows, float *de_rows,
                                   int distinct, hipStream_t st);
hipError_t launch_loss_reduce(const double *partials, int n, double *loss_out, hipStream_t st);
// the N3 regulariser (okge_n3.hip): value partials + gradient of c sum |x|^3 over the candidate rows (cand_wgs workgroups,
// none at cand_passes == 0) and the 2 B prefix rows; the caller reduces the partials (launch_loss_reduce)
struct N3Args {
    const float   *E, *R;
    float         *dE, *dR;          // the tables' gradients; row_grads: the occurrence rows gE [N + B][d] / gR [B][d]
    double        *partial;          // [cand_wgs + prefix_wgs]
    const int32_t *cand_ids;
    PrefixDev      p;
    DropDev        drop_c;
    double         value_cand, value_prefix;   // c * passes, c: what a workgroup's sum of |x|^3 is multiplied by
    double         grad_cand, grad_prefix;     // 3 c passes / normalizer, 3 c / normalizer (the mask scale joins in the kernel)
    int32_t        cand_first, N, n_ent, d, n_oct, rows_per_wg, cand_wgs, wg0;
    int32_t        vec;              // d % 4 == 0 and every base 16-byte aligned: float4 accesses
    int32_t        loss_only, row_grads, cand_atomic, prefix_atomic;
};
hipError_t launch_n3(const N3Args &a, int wg0, int n_wgs, hipStream_t st);     // workgroups [wg0, wg0 + n_wgs) of the call
hipError_t launch_kl_count_pos(const int32_t *pos_row, int nnz, int Bpad, float *row_ysum, hipStream_t st);
hipError_t launch_kl_row_lse(const float *stats, int tiles, int B, int Bpad, float *run, int first, int last, float *row_lse,
                             hipStream_t st, const int32_t *pos_row = nullptr, int nnz = 0, float *row_ysum = nullptr);
hipError_t launch_encode_rows(const float *table, int64_t table_rows, int d, const int32_t *ids, int first_id, int n,
                              const DropDev &drop, float *out, int64_t ld_out, int *id_err, hipStream_t st);
// log-sum-exp over `world` per-shard row log-sum-exps: out[b] = log sum_r exp(parts[r][b])  (sharded KL loss)
hipError_t launch_merge_lse(const float *parts, int world, int B, float *out, hipStream_t st);
// backward of the prefix scores from a dense (b, n) gradient block, and the scatter of encoded-row gradients (okge_gemm.hip)
size_t score_backward_workspace_bytes(int b, int n, int d);
hipError_t launch_score_backward(int scorer, int sp, const float *G, int64_t ld_g, int b, int n, const float *ent, int64_t ld_ent,
                                 const float *rel, int64_t ld_rel, const float *cand, int64_t ld_cand, int d, float *d_ent,
                                 float *d_rel, float *d_cand, void *workspace, hipStream_t st);
hipError_t launch_scatter_rows(const float *rows, int64_t ld, const int32_t *ids, const int32_t *order, int first_id, int n, int d,
                               const DropDev &drop, float *table, int64_t table_rows, int *id_err, hipStream_t st);
// error text for okge_last_error(), shared by the translation units of the C ABI (defined in okge_api.hip)
int report_error(int code, const std::string &msg);

// token-pooled embedder (okge_pool.hip): one _encode call of a batch (UnigramPoolingRelationEmbedder._encode, model.py:762-786)
constexpr int POOL_MAX_CALLS = 8;
struct PoolCall {
    const float   *W;                       // token table (vocab x d)
    const int32_t *tokens;                  // (n_ids x L) token ids
    const int32_t *ids;                     // rows of the call (or first_id + i)
    float         *raw, *out;               // [n][ld] pooled rows / normalised rows (out == raw without batch-norm)
    float         *saved;                   // [4 d] {mean, rstd, scratch, scratch} of this call; nullptr: no training-mode batch-norm
    const float   *dY;                      // backward: [n][ld] gradient of `out`
    const float   *bn_weight, *bn_bias;     // nullptr: no batch-norm
    float         *run_mean, *run_var;
    float         *d_weight, *d_bias, *dW;  // backward targets
    float         *partial;                 // [ceil(n / 32)][2][d] scratch of this call
    uint8_t       *touched;                 // backward: [vocab] bytes, touched[token] = touched_stamp for every row of dW written (or nullptr)
    float         *sumW;                    // catch-up (okge_pool_catch_up_calls): Adagrad accumulator of W and
    int32_t       *steps;                   //   [vocab] optimizer steps each row of W has seen
    int64_t        ld;
    int32_t        d, L, first_id, n, pool, n_ids, vocab, touched_stamp;
    float          eps, momentum;
};
size_t pool_workspace_bytes(int n, int d);
hipError_t launch_pool_encode_calls(const PoolCall *calls, int n_calls, int training, int *id_err, hipStream_t st);
// rows of W the calls' tokens name: their pending decay-only Adagrad steps (okge_adagrad_lazy), before the forward reads them
hipError_t launch_pool_catch_up(const PoolCall *calls, int n_calls, const int32_t *counters, float lr, float wd, float eps, int *id_err,
                                hipStream_t st);
// state == nullptr: the token-table gradient is scattered with float atomics; otherwise (pool sum / mean, slot sizes that are
// a multiple of 4): store-and-sum through a device-built inverted index, bit-reproducible (okge_pool.hip, "scatter plan")
size_t pool_scatter_state_bytes(const PoolCall *calls, int n_calls);
size_t pool_scatter_workspace_bytes(const PoolCall *calls, int n_calls);
hipError_t launch_pool_backward_calls(const PoolCall *calls, int n_calls, int *id_err, hipStream_t st, void *state = nullptr,
                                      size_t state_bytes = 0, void *scratch = nullptr, size_t scratch_bytes = 0);
// LSTM token encoder (okge_lstm.hip): the bodies of the C ABI's okge_lstm_* (okge.h), err = the device's id-error word
size_t lstm_workspace_bytes(int32_t rows, int32_t max_len, int32_t d, int32_t training);
int lstm_encode_calls(const okge_lstm_slot *s, const okge_lstm_call *calls, int32_t n_calls, int32_t training, float *raw, float *out,
                      int64_t ld, int32_t *pos_tok, void *workspace, size_t workspace_bytes, int *err, void *stream);
int lstm_backward_calls(const okge_lstm_slot *s, const okge_lstm_call *calls, int32_t n_calls, const float *raw, const float *d_out,
                        int64_t ld, const int32_t *pos_tok, const int32_t *pos_order, float *dW, float *d_w_ih, float *d_w_hh,
                        float *d_b_ih, float *d_b_hh, float *d_bn_weight, float *d_bn_bias, void *workspace, size_t workspace_bytes,
                        int *err, void *stream);
// Bigram token encoder (okge_bigram.hip): the bodies of the C ABI's okge_bigram_* (okge.h), err = the device's id-error word
size_t bigram_workspace_bytes(int32_t rows, int32_t max_len, int32_t d, int32_t training);
int bigram_encode_calls(const okge_bigram_slot *s, const okge_bigram_call *calls, int32_t n_calls, int32_t training, float *out, int64_t ld,
                        int32_t *pos_tok, void *workspace, size_t workspace_bytes, int *err, void *stream);
int bigram_backward_calls(const okge_bigram_slot *s, const okge_bigram_call *calls, int32_t n_calls, const float *d_out, int64_t ld,
                          const int32_t *pos_tok, const int32_t *pos_order, float *dW, float *d_conv, float *d_bn_weight,
                          float *d_bn_bias, void *workspace, size_t workspace_bytes, int *err, void *stream);
// Lookup embedder variants (okge_lookup_encode.hip): the bodies of the C ABI's okge_lookup_* (okge.h), err = the device's id-error word
size_t lookup_workspace_bytes(int32_t ent_rows, int32_t rel_rows, int32_t d, int32_t training);
int lookup_encode_calls(const okge_lookup_encoder *e, const okge_lookup_call *calls, int32_t n_calls, int32_t training, float *EV,
                        int64_t ld_e, float *RV, int64_t ld_r, void *workspace, size_t workspace_bytes, int *err, void *stream);
int lookup_backward_calls(const okge_lookup_encoder *e, const okge_lookup_call *calls, int32_t n_calls, const float *EV, int64_t ld_e,
                          const float *RV, int64_t ld_r, const float *dEV, int64_t ld_de, const float *dRV, int64_t ld_dr,
                          const int32_t *list_order, int32_t n_list, float *dE, float *dR, float *d_bn_e_weight, float *d_bn_e_bias,
                          float *d_bn_r_weight, float *d_bn_r_bias, float *dW_obj, float *dW_subj, void *workspace,
                          size_t workspace_bytes, int *err, void *stream);
// Tucker3 / RESCAL fold and backward (okge_tucker3.hip); cus = compute units of the device (split of the long contractions)
int tucker3_splits(int B, int Nn, int outer, int cus);
size_t tucker3_workspace_bytes(int B, int d, int r, int cus);
hipError_t launch_tucker3_fold(const float *W, const float *x, int64_t ld_x, const float *rho, int64_t ld_r, int n_po, int B, int d, int r,
                               int transpose, float *out, int rows_out, int64_t ld_out, int cols_out, float *slab, int cus, hipStream_t st);
hipError_t launch_tucker3_backward(const float *W, const float *ent, int64_t ld_e, const float *rho, int64_t ld_r, const float *dq,
                                   int64_t ld_q, int n_po, int B, int d, int r, int fresh, float *d_ent, float *d_rel, float *dW,
                                   float *slab, int cus, hipStream_t st);
hipError_t launch_tucker3_triples(const float *W, const float *subj, int64_t ld_s, const float *rho, int64_t ld_r, const float *obj,
                                  int64_t ld_o, int n, int d, int r, float *q, float *slab, float *out, int cus, hipStream_t st);
hipError_t launch_tucker3_apply(const float *M, int64_t ld_m, const float *x, int64_t ld_x, int n, int d, int transpose, float *out,
                                int64_t ld_out, hipStream_t st);
hipError_t launch_tucker3_outer(const float *u, int64_t ld_u, const float *v, int64_t ld_v, int n, int d, float *out, int64_t ld_out,
                                hipStream_t st);
// ---- okge_optim.hip: the dense optimizer, clipping and scaling launches -----------------------------------------------------
hipError_t launch_scale(float *x, int64_t n, const float *alpha_dev, hipStream_t st);
hipError_t launch_rescale2(float *x0, int64_t n0, float *x1, int64_t n1, const float *alpha_dev, float applied, hipStream_t st);
hipError_t launch_adagrad(float *p, float *g, float *sum, int64_t n, float lr, float wd, float eps, int zero_grad,
                          hipStream_t st);
hipError_t launch_adagrad2(float *p0, float *g0, float *s0, int64_t n0, float *p1, float *g1, float *s1, int64_t n1,
                           float lr, float wd, float eps, int zero_grad, hipStream_t st);
// torch.nn.utils.clip_grad_norm_ over two gradient tensors: coef = min(1, max_norm / (||g|| + 1e-6)) -> coef_dev (fp32),
// ||g|| -> norm_dev (double); the caller scales with launch_scale (trainer.py:236-240)
hipError_t launch_clip_coef(const float *g0, int64_t n0, const float *g1, int64_t n1, float max_norm, double *partial,
                            int n_partial, float *coef_dev, double *norm_dev, hipStream_t st);
// the same over up to eight gradient tensors, three launches: n_partial partial sums (a fixed grid: which workgroup sums which
// element depends on the sizes alone), the coefficient, the scaling (nothing but the coefficient is read when it is 1).  A tensor
// may come with a touched-row byte map: rows whose byte differs from `stamp` are neither read nor written
constexpr int CLIP_MAX_SEGS = 8;
struct GradSeg { float *g; int64_t n; const uint8_t *touched; int32_t row_len, stamp; };
hipError_t launch_clip_multi(const GradSeg *segs, int n_segs, float max_norm, double *partial, int n_partial, float *coef_dev,
                             double *norm_dev, hipStream_t st);
// dense Adagrad over up to four tensors in one launch; a tensor may come with a touched-row byte map (rows whose byte differs
// from `stamp` hold an all-zero gradient by contract: it is neither read nor cleared)
constexpr int ADAGRAD_MAX_SEGS = 4;
struct AdagradSegM { float *p, *g, *s; int64_t n; const uint8_t *touched; int32_t row_len, stamp, zero_grad; };
hipError_t launch_adagrad_multi(const AdagradSegM *segs, int n_segs, float lr, float wd, float eps, hipStream_t st);
// deferred weight-decay-only updates (okge_adagrad_lazy): steps == nullptr: a plain dense tensor of rows * row_len floats
constexpr int LAZY_STEP = 0, LAZY_FLUSH = 1;
struct LazySeg { float *p, *g, *s; int32_t *steps; uint8_t *touched; int64_t rows; int32_t row_len, stamp; };
hipError_t launch_adagrad_lazy(const LazySeg *segs, int n_segs, int32_t *counters, int window, int mode, float lr, float wd,
                               float eps, hipStream_t st);
// ---- okge_adam.hip: dense Adam over one or two tensors.  state: device int32[4] per tensor = { t, bits of c1 / c2 / the sparse
// step size }; the prologue (one workgroup) advances every distinct state by one step and forms the three scalars of the new t
constexpr int ADAM_MAX_SEGS = 2;
struct AdamSeg { float *p, *g, *m, *v; const int32_t *state; int64_t n; };
constexpr int ADAM_MULTI_MAX_SEGS = 4;
struct AdamStates { int32_t *state[ADAM_MULTI_MAX_SEGS]; int n; };
hipError_t launch_adam_prologue(int32_t *const *states, int n_states, float lr, float beta1, float beta2, hipStream_t st);
hipError_t launch_adam2(const AdamSeg &a, const AdamSeg &b, float beta1, float beta2, float eps, float wd, int zero_grad, hipStream_t st);
// dense Adam over up to four tensors in one launch, gradients cleared in the sweep; a tensor may come with a touched-row byte map
// (AdagradSegM's contract: a row whose byte differs from `stamp` takes the update with g = 0, its gradient row neither read nor cleared)
struct AdamSegM { float *p, *g, *m, *v; const int32_t *state; int64_t n; const uint8_t *touched; int32_t row_len, stamp; };
hipError_t launch_adam_multi(const AdamSegM *segs, int n_segs, float beta1, float beta2, float eps, float wd, hipStream_t st);
// row-sparse training (okge_sparse.hip).  Gather: the occurrence rows of one batch -- candidates, prefix entities, relations --
// as the two small tables EV (N + B rows) / RV (B rows) of the relabelled problem, and the position ids that name them
// (pos_ids[0..B) = N + i, pos_ids[B..2B) = i).
struct RowsGather {
    const float   *E, *R;
    float         *EV, *RV;
    const int32_t *cand_ids, *po_obj, *sp_subj, *po_rel, *sp_rel;
    int32_t       *pos_ids;
    int           *id_err;
    int64_t        n_ent, n_rel;
    int32_t        cand_first, N, n_po, n_sp, d, vec;
};
hipError_t launch_rows_gather(const RowsGather &a, hipStream_t st);
// okge_adagrad_rows: one segment per tensor.  keys[0] / keys[1]: n 8-byte sort keys each (ping-pong of the merge passes)
constexpr int ROWS_MAX_SEGS = 2;
struct RowsSeg {
    float         *p, *s;
    const float   *g;
    const int32_t *ids;
    uint64_t      *keys[2];
    int64_t        ld_g;
    int32_t        n, table_rows, row_len, vec, lane_shift;      // 1 << lane_shift lanes share one run of equal ids
    int32_t       *steps;                                        // okge_adagrad_rows_decay: [table_rows] optimizer steps each row has seen
    float         *s2;                                           // okge_adam_rows: s = exp_avg, s2 = exp_avg_sq,
    const int32_t *state;                                        //   state = the tensor's device state (AdamSeg)
};
struct RowsSegs { RowsSeg s[ROWS_MAX_SEGS]; int n_segs; int *id_err; };
hipError_t launch_rows_sort(const RowsSegs &segs, int *sorted_in, hipStream_t st);
hipError_t launch_rows_update(const RowsSegs &segs, int sorted_in, float lr, float eps, hipStream_t st);
// okge_adam_rows: the same heads and the same walk with the sparse Adam body; the step size is read from each segment's state
hipError_t launch_rows_update_adam(const RowsSegs &segs, int sorted_in, float beta1, float beta2, float eps, hipStream_t st);
// okge_rows_to_dense: the same heads and the same walk; the coalesced row is stored to (accumulate: continued from) row `id` of the
// dense gradient table seg.p -- seg.s is not read
hipError_t launch_rows_to_dense(const RowsSegs &segs, int sorted_in, int accumulate, hipStream_t st);
// deferred weight decay on the row-sparse step (okge_rows_catch_up / okge_adagrad_rows_decay): every segment 16-byte accessible
// (vec) with a step counter per table row; counters[0] = T, the optimizer steps taken
hipError_t launch_rows_update_decay(const RowsSegs &segs, int sorted_in, const int32_t *counters, float lr, float wd, float eps,
                                    hipStream_t st);
struct RowsCatchSeg { float *p, *s; int32_t *steps; const int32_t *ids; int32_t n, table_rows, row_len, _pad; };
struct RowsCatchSegs { RowsCatchSeg s[ROWS_MAX_SEGS]; int n_segs; int64_t wave0[ROWS_MAX_SEGS + 1]; };
hipError_t launch_rows_catch_up(const RowsCatchSeg *segs, int n_segs, const int32_t *counters, float lr, float wd, float eps,
                                hipStream_t st);
hipError_t launch_dc_reduce(const float *slab, int nsplit, int rows_pad, int D16, int N, int d, const int32_t *cand_ids,
                            int cand_first, int exclusive, int grads_zero, float *dE, int64_t table_rows, int *id_err,
                            hipStream_t st);
// sums the partial candidate-gradient slabs of a stream-K launch of fused_tile64k_kernel (slab 2p / 2p+1 = first / last
// segment of workgroup p; tiles covered by one whole segment were stored by the tile kernel itself)
hipError_t launch_dc_reduce_streamk(const float *slab, int tiles, int chunks_per_tile, int workgroups, int D16, int N, int d,
                                    const int32_t *cand_ids, int cand_first, int exclusive, int grads_zero, float *dE,
                                    int64_t table_rows, int *id_err, hipStream_t st);
hipError_t launch_score_triples(const float *S, int64_t lds_, const float *Rr, int64_t ldr, const float *O, int64_t ldo,
                                int n, int d, int scorer, float *out, hipStream_t st);
// ---- okge_rank.hip: evaluation's rank launches --------------------------------------------------------------------------------
hipError_t launch_rank_metrics(const int64_t *ranks, int64_t n, double *acc, hipStream_t st);
// fused evaluation (okge_evaluate_fused): point scores in the tile kernel's summation order, then ranks from the counts
// fused evaluation: the two small kernels around the tile sweep
struct EvalPointsArgs {
    const float   *E, *R;
    PrefixDev      p;
    float         *Q;                      // [Bpad][ldq] folded queries at their SORTED positions
    const int32_t *cand_ids;
    const int64_t *row_ptr, *grp_ptr, *filt_ptr;
    const int32_t *ids, *filt_col;
    float         *true_out, *filt_x;      // [n_groups] (sorted numbering), [n_filter]
    int64_t       *row_ptr_sorted, *gshift;
    int32_t       *group_row;              // [n_groups] row of every group (original numbering), for eval_ranks
    int64_t        table_rows;
    int32_t        d, scorer, ldq, KB, Bpad, cand_first, n_cand;
    // candidate-sharded evaluation (okge_evaluate_fused_shard): the queries arrive folded (original row order), the local
    // candidates are the global columns col_lo .. col_lo + n_cand - 1 of n_cand_global; ids / filter columns stay global
    const float   *Q_in;                   // [B][ldq] or nullptr (fold from E / R: the single-device path)
    int32_t        col_lo, n_cand_global;
};
struct EvalRanksArgs {
    const int32_t  *counts;                // [n_groups][2] (atomics path) or nullptr
    const uint32_t *slab;                  // [tiles][n_groups] packed counts or nullptr
    const float    *true_scores, *filt_x;
    const int64_t  *filt_ptr, *gshift;
    const int32_t  *group_row;
    int64_t        *ranks;
    double         *acc;
    int64_t        *counts_out;            // sharded: [n_groups][2] {#greater, #equal} of THIS shard instead of ranks + meters
    int64_t         n_groups;
    int32_t         tiles, B;
};
// either part may be absent (nullptr): points of one batch and ranks of ANOTHER share a launch in a run of batches
hipError_t launch_eval_side(const EvalPointsArgs *pts, const EvalRanksArgs *rk, hipStream_t st);
// ---- the validation loss of an evaluation batch (okge_evaluate_*_loss) ----
// the label term, left by the points launch at the rows' SORTED positions: sum of the scores of the row's distinct positive
// columns and their number
struct EvalLossPoints { double *pos_sum; int32_t *npos; };
// the same launch as launch_eval_side with the loss variant of the points part (a kernel of its own: the no-loss launch is
// what it was)
hipError_t launch_eval_side_loss(const EvalPointsArgs *pts, const EvalLossPoints *el, const EvalRanksArgs *rk, hipStream_t st);
// Per row, the tiles' partials merged in tile order and joined with the label term (a launch over the rows; part == nullptr:
// rows[] holds the rows' losses already); then, in a one-workgroup launch, the rows added in row order into *out.
struct EvalLossReduce {
    const float2  *part;        // [tiles][Bpad] (sum softplus, sum x) or (max, sum-exp) per (tile, row)
    const double  *pos_sum;     // [B]
    const int32_t *npos;        // [B]
    double        *rows;        // [B] scratch: the rows' losses
    double        *out;
    double         smoothing;   // BCE label smoothing
    int32_t        tiles, B, Bpad, N, kind;   // kind: LOSS_BCE / LOSS_KL
};
hipError_t launch_eval_loss_reduce(const EvalLossReduce &a, hipStream_t st);
// the rows' losses of a materialised score block (one workgroup per row) -> rows[B]; launch_eval_loss_reduce adds them up
hipError_t launch_block_loss_rows(const float *scores, int64_t ld, int B, int N, const int64_t *row_ptr, const int64_t *grp_ptr,
                                  const int32_t *ids, int kind, double smoothing, double *rows, hipStream_t st);
hipError_t launch_ranks(const float *scores, int64_t ld, int B, int N, const int64_t *filt_ptr,
                        const int32_t *filt_col, const int64_t *row_ptr, const int64_t *grp_ptr, const int32_t *ids,
                        int64_t *ranks, int col0, const float *true_in, float *true_out, int64_t *counts_out,
                        hipStream_t st);
// top-k link prediction (okge_topk.hip).  Cut: the per-tile records of fused_tile_kernel<KB, MODE_TOPK> from a materialised
// score block X[B][ldx] of N local candidates (slot sizes above 256).  Merge: per row, L lists of kq records + the running
// (B, k) list -> the running list, in the total order of okge_topk.h.
hipError_t launch_topk_cut(const float *X, int64_t ldx, int B, int Bpad, int N, int cand_col0, const int64_t *filt_ptr,
                           const int32_t *filt_col, int kq, TopkRec *part, hipStream_t st);
struct TopkMergeArgs {
    const float   *sc;          // record (list l, row b, slot s) is element ((l * rows_ld + b) * kq + s) * elem_stride of sc / cl
    const int32_t *cl;
    int32_t        elem_stride, L, rows_ld, kq, B, k;
    int32_t        first;       // 1: the running list starts empty; 0: it is read from out_*
    float         *out_sc;      // [B][k]
    int32_t       *out_cl;
    int32_t       *out_id;      // optional: entity id of every column (cand_ids[col] or cand_first + col; -1 for padding)
    const int32_t *cand_ids;
    int32_t        cand_first;
};
hipError_t launch_topk_merge(const TopkMergeArgs &a, hipStream_t st);

}  // namespace okge
