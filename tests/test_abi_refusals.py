"""CPU-only: every refusal of the C ABI's host layer (csrc/okge_core.hip and the okge_api_*.hip units) that is reached before
the first HIP call, pinned by return code AND by the exact okge_last_error() text.  A table of deliberately bad calls through
_native.lib(): pointers a refusal path only compares against NULL point at a small host buffer, and no row gets as far as
id_err_ptr(), an event or a launch.  The workspace-size answers are pinned by test_launch_plan.py and test_wide_plan.py."""
import ctypes
from ctypes import addressof, byref, c_void_p

import pytest

from open_knowledge_graph_embeddings_amd import _native as nv

INV, UNS, WS = -1, -2, -3
CLEAR_GRADS, ROW_GRADS, LOSS_ONLY = nv.OKGE_TRAIN_CLEAR_GRADS, nv.OKGE_TRAIN_ROW_GRADS, nv.OKGE_TRAIN_LOSS_ONLY
BIAS_R, BIAS_E = nv.OKGE_BIAS_RELATION, nv.OKGE_BIAS_ENTITY

_RAW = (ctypes.c_char * 4096)()
P = (addressof(_RAW) + 255) & ~255          # a 256-byte aligned host address: compared against NULL / tested for alignment only
P4 = P + 4                                  # 4-byte aligned only
_KEEP = []
HUGE = 1 << 40                              # a workspace size no layout exceeds (the pointer is never dereferenced)

D512_TILE = ("slot sizes above 512 are not supported by the tile kernels: slot sizes 513 to 4096 run through okge_score_prefixes, "
             "okge_train_forward_backward (dense gradients) and okge_evaluate_batch")
D512_TRAIN_TILES = ("slot sizes above 512 are not supported by the tile kernels: the sharded phases stop there, the unsharded "
                    "okge_train_forward_backward takes slot sizes up to 4096")
D512_QUERY_CALL = ("slot sizes above 512 are not supported by the tile kernels: the sharded phases stop there, the unsharded "
                   "okge_score_prefixes / okge_train_forward_backward take slot sizes up to 4096")
D512_EVAL = ("slot sizes above 512 are not supported by the tile kernels: fused evaluation stops there, okge_evaluate_batch "
             "(PipelinedEvaluator) takes slot sizes up to 4096")
SHARD_RANGE = "shard range must cover exactly the rows of the local entity table"
LOCAL_RANGE = "candidate range outside the local entity table"
CLEAR_MSG = "OKGE_TRAIN_CLEAR_GRADS needs a contiguous candidate range on an unsharded table"
TRAIN_TABLE = "training needs candidates from the entity table"
TOPK_TABLE = "top-k takes its candidates from the entity table"
EVAL_MODE = "fused evaluation is the eval-mode path (no dropout, candidates from the entity table)"
POOL_1_8 = "1 to 8 pooled calls per batch"
ALIGN16 = "adagrad buffers must be 16-byte aligned"
STAMP = "touched_stamp must lie in 1..255"
TUCKER_WS = "workspace too small or unaligned (okge_tucker3_workspace_bytes)"
ROWS_WS = "workspace too small (okge_adagrad_rows_workspace_bytes)"


def tables(d=16, scorer=nv.OKGE_COMPLEX, n_ent=100, n_rel=10, E=P, R=P):
    return nv.Tables(E, R, n_ent, n_rel, d, scorer)


def batch(n_po=2, n_sp=2, po_rel=P, po_obj=P, sp_subj=P, sp_rel=P, drop=0.0):
    b = nv.PrefixBatch(po_rel, po_obj, sp_subj, sp_rel, n_po, n_sp)
    b.drop_po_ent.p = drop
    return b


def cand(n=50, first_id=0, ids=None, table=None, table_rows=0, drop=0.0):
    c = nv.Candidates(ids, first_id, n)
    c.drop.p = drop
    c.table, c.table_rows = table, table_rows
    return c


def pos(nnz=1, col=P, row=P):
    return nv.Positives(col, row, nnz)


def shard(lo=0, hi=100, col0=0):
    return nv.Shard(lo, hi, col0, 0)


def embedder(W=P, tok=P, vocab=20, d=8, n_ids=30, max_len=4, pool=0, bn=False, **kw):
    e = nv.TokenEmbedder(W, tok, vocab, d, n_ids, max_len, pool)
    _KEEP.append(e)                         # a pooled call holds only its address
    if bn:
        e.bn_weight, e.bn_bias, e.bn_running_mean, e.bn_running_var = P, P, P, P
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def pool_call(e, n=5, first_id=0, ids=None, raw=P, out=P + 1024, ld=8, **kw):
    c = nv.PoolCall(ctypes.pointer(e), ids, first_id, n, raw, out, ld)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def arr(kind, *items):
    return (kind * len(items))(*items)


def adagrad_t(p=P, g=P, s=P, n=16, touched=None, row_len=0, stamp=0, zero_grad=0):
    return nv.AdagradTensor(p, g, s, n, touched, row_len, stamp, zero_grad)


def lazy_t(p=P, g=P, s=P, rows=4, steps=None, touched=None, row_len=4, stamp=0):
    return nv.LazyTensor(p, g, s, rows, steps, touched, row_len, stamp)


def rows_t(p=P, s=P, ids=P, g=P, ld_g=4, n=3, table_rows=10, row_len=4):
    return nv.RowsTensor(p, s, ids, g, ld_g, n, table_rows, row_len)


def decay_t(p=P, s=P, ids=P, g=P, ld_g=4, steps=P, n=3, table_rows=10, row_len=4):
    return nv.RowsDecayTensor(p, s, ids, g, ld_g, steps, n, table_rows, row_len)


ROWS = []


def row(name, fn, args, rc, msg):
    ROWS.append(pytest.param(fn, args, rc, msg, id=name))


def R(x):
    return byref(x) if x is not None else None


# ---- check_common, through okge_score_prefixes (the entry point with a wide path) -------------------------------------------
def score(t=None, b=None, c=None, scores=P, ld=64, ws=P, ws_bytes=HUGE):
    return (R(t), R(b), R(c), scores, ld, ws, ws_bytes, None)


row("common-null-descriptor", "okge_score_prefixes", score(None, batch(), cand()), INV, "null descriptor")
row("common-null-batch", "okge_score_prefixes", score(tables(), None, cand()), INV, "null descriptor")
row("common-null-cand", "okge_score_prefixes", score(tables(), batch(), None), INV, "null descriptor")
row("common-null-table", "okge_score_prefixes", score(tables(E=None), batch(), cand()), INV, "null embedding table")
row("common-null-rel-table", "okge_score_prefixes", score(tables(R=None), batch(), cand()), INV, "null embedding table")
row("common-bad-shape", "okge_score_prefixes", score(tables(d=0), batch(), cand()), INV, "bad table shape")
row("common-no-relations", "okge_score_prefixes", score(tables(n_rel=0), batch(), cand()), INV, "bad table shape")
row("common-unknown-scorer", "okge_score_prefixes", score(tables(scorer=7), batch(), cand()), INV, "unknown scorer")
row("common-odd-complex", "okge_score_prefixes", score(tables(d=15), batch(), cand()), INV, "ComplEx needs an even slot size")
row("common-d-4098", "okge_score_prefixes", score(tables(d=4098), batch(), cand()), UNS, "slot sizes above 4096 are not supported")
row("common-bias-wide", "okge_score_prefixes", score(tables(d=516, scorer=BIAS_R), batch(), cand()), UNS,
    "the data-bias scorers stop at slot size 512: the wide path is built for ComplEx and DistMult")
row("common-empty-batch", "okge_score_prefixes", score(tables(), batch(0, 0), cand()), INV, "empty batch")
row("common-negative-batch", "okge_score_prefixes", score(tables(), batch(-1, 3), cand()), INV, "empty batch")
row("common-null-po", "okge_score_prefixes", score(tables(), batch(po_rel=None), cand()), INV, "null po ids")
row("common-null-sp", "okge_score_prefixes", score(tables(), batch(sp_rel=None), cand()), INV, "null sp ids")
row("common-no-candidates", "okge_score_prefixes", score(tables(), batch(), cand(n=0)), INV, "no candidates")
row("common-range", "okge_score_prefixes", score(tables(), batch(), cand(n=50, first_id=60)), INV,
    "candidate range outside the candidate table")
row("common-range-own-table", "okge_score_prefixes", score(tables(), batch(), cand(n=50, table=P, table_rows=10)), INV,
    "candidate range outside the candidate table")
row("score-null-scores", "okge_score_prefixes", score(tables(), batch(), cand(), scores=None), INV, "bad scores buffer")
row("score-short-ld", "okge_score_prefixes", score(tables(), batch(), cand(), ld=49), INV, "bad scores buffer")
row("score-workspace", "okge_score_prefixes", score(tables(), batch(), cand(), ws_bytes=16), WS, "workspace too small")
row("score-null-workspace", "okge_score_prefixes", score(tables(), batch(), cand(), ws=None), WS, "workspace too small")
row("score-wide-workspace", "okge_score_prefixes", score(tables(d=516), batch(), cand(), ws_bytes=16), WS, "workspace too small")


# ---- top-k ------------------------------------------------------------------------------------------------------------------
def topk(t, b, c, k=5, filt_ptr=None, filt_col=None, n_filter=0, range_n=0, out_sc=P, out_cl=P, out_id=P, ws=P, ws_bytes=HUGE):
    return (R(t), R(b), R(c), k, filt_ptr, filt_col, n_filter, range_n, out_sc, out_cl, out_id, ws, ws_bytes, None)


row("common-d-516-no-wide-path", "okge_topk_prefixes", topk(tables(d=516), batch(), cand()), UNS, D512_TILE)
row("topk-bias", "okge_topk_prefixes", topk(tables(scorer=BIAS_R), batch(), cand()), UNS,
    "okge_topk_prefixes does not take the OKGE_BIAS_RELATION scorer: predictions are built for the ComplEx and DistMult scorers")
row("topk-k-0", "okge_topk_prefixes", topk(tables(), batch(), cand(), k=0), INV, "k must be at least 1")
row("topk-k-65", "okge_topk_prefixes", topk(tables(), batch(), cand(), k=65), UNS, "top-k keeps at most 64 candidates per row")
row("topk-cand-table", "okge_topk_prefixes", topk(tables(), batch(), cand(table=P, table_rows=100)), UNS, TOPK_TABLE)
row("topk-batch-dropout", "okge_topk_prefixes", topk(tables(), batch(drop=0.5), cand()), UNS, "top-k is an eval-mode call: no dropout")
row("topk-cand-dropout", "okge_topk_prefixes", topk(tables(), batch(), cand(drop=0.5)), UNS, "top-k is an eval-mode call: no dropout")
row("topk-filter", "okge_topk_prefixes", topk(tables(), batch(), cand(), n_filter=3), INV, "bad filter / range")
row("topk-range", "okge_topk_prefixes", topk(tables(), batch(), cand(), range_n=-1), INV, "bad filter / range")
row("topk-null-scores", "okge_topk_prefixes", topk(tables(), batch(), cand(), out_sc=None), INV, "null output")
row("topk-null-ids", "okge_topk_prefixes", topk(tables(), batch(), cand(), out_id=None), INV, "null output")
row("topk-workspace", "okge_topk_prefixes", topk(tables(), batch(), cand(), ws_bytes=16), WS, "workspace too small")


def topk_q(t, sh, c, Q=P, ldq=64, B=4, k=5, n_filter=0, range_n=0, out_sc=P, out_cl=P, ws=P, ws_bytes=HUGE):
    return (R(t), R(sh), Q, ldq, B, R(c), k, None, None, n_filter, range_n, out_sc, out_cl, ws, ws_bytes, None)


row("topk-queries-cand-table", "okge_topk_queries", topk_q(tables(), shard(), cand(table=P, table_rows=100)), UNS, TOPK_TABLE)
row("topk-queries-bad-tables", "okge_topk_queries", topk_q(None, shard(), cand()), INV, "bad tables")
row("topk-queries-d-516", "okge_topk_queries", topk_q(tables(d=516), shard(), cand(), ldq=512), UNS, D512_QUERY_CALL)
row("topk-queries-k-65", "okge_topk_queries", topk_q(tables(), shard(), cand(), k=65), UNS, "top-k keeps at most 64 candidates per row")
row("topk-queries-dropout", "okge_topk_queries", topk_q(tables(), shard(), cand(drop=0.25)), UNS, "top-k is an eval-mode call: no dropout")
row("topk-queries-null-cols", "okge_topk_queries", topk_q(tables(), shard(), cand(), out_cl=None), INV, "null output")
row("topk-queries-workspace", "okge_topk_queries", topk_q(tables(), shard(), cand(), ws=None), WS, "workspace too small")
row("topk-merge-lists", "okge_topk_merge", (None, P, 2, 4, 5, P, P, None), INV, "bad lists")
row("topk-merge-no-lists", "okge_topk_merge", (P, P, 0, 4, 5, P, P, None), INV, "bad lists")
row("topk-merge-k-0", "okge_topk_merge", (P, P, 2, 4, 0, P, P, None), INV, "k must be at least 1")
row("topk-merge-k-65", "okge_topk_merge", (P, P, 2, 4, 65, P, P, None), UNS, "top-k keeps at most 64 candidates per row")


# ---- training: train_core (d = 16) and wide_core (d = 516) ------------------------------------------------------------------
def train(t, b, c, p, loss=nv.OKGE_LOSS_BCE, norm=1.0, flags=0, loss_out=P, dE=P, dR=P, scores=None, ld=0, ws=P, ws_bytes=HUGE):
    return (R(t), R(b), R(c), R(p), loss, 0.0, norm, flags, loss_out, dE, dR, scores, ld, ws, ws_bytes, None)


for d in (16, 516):
    T, w = "okge_train_forward_backward", "train-d%d-" % d
    row(w + "null-dR", T, train(tables(d=d), batch(), cand(), pos(), dR=None), INV, "null output")
    row(w + "null-positives", T, train(tables(d=d), batch(), cand(), None), INV, "bad positives")
    row(w + "negative-nnz", T, train(tables(d=d), batch(), cand(), pos(nnz=-1)), INV, "bad positives")
    row(w + "null-pos-col", T, train(tables(d=d), batch(), cand(), pos(col=None)), INV, "bad positives")
    row(w + "unknown-loss", T, train(tables(d=d), batch(), cand(), pos(), loss=5), INV, "unknown loss")
    row(w + "null-loss-out", T, train(tables(d=d), batch(), cand(), pos(), loss_out=None), INV, "null output")
    row(w + "null-dE", T, train(tables(d=d), batch(), cand(), pos(), dE=None), INV, "null output")
    row(w + "cand-table", T, train(tables(d=d), batch(), cand(table=P, table_rows=100), pos()), INV, TRAIN_TABLE)
    row(w + "normalizer-0", T, train(tables(d=d), batch(), cand(), pos(), norm=0.0), INV, "normalizer must be positive")
    row(w + "normalizer-nan", T, train(tables(d=d), batch(), cand(), pos(), norm=float("nan")), INV, "normalizer must be positive")
    row(w + "short-scores", T, train(tables(d=d), batch(), cand(), pos(), scores=P, ld=49), INV, "bad scores buffer")
    row(w + "workspace", T, train(tables(d=d), batch(), cand(), pos(), ws_bytes=16), WS, "workspace too small")
    row(w + "null-workspace", T, train(tables(d=d), batch(), cand(), pos(), ws=None), WS, "workspace too small")
    row(w + "clear-grads-id-list", T, train(tables(d=d), batch(), cand(ids=P), pos(), flags=CLEAR_GRADS), INV, CLEAR_MSG)
row("train-d16-row-grads-loss-only", T, train(tables(), batch(), cand(), pos(), flags=ROW_GRADS | LOSS_ONLY), INV,
    "OKGE_TRAIN_ROW_GRADS asks for gradients: not with OKGE_TRAIN_LOSS_ONLY")
row("train-d516-row-grads", T, train(tables(d=516), batch(), cand(), pos(), flags=ROW_GRADS), UNS,
    "OKGE_TRAIN_ROW_GRADS stops at slot size 512: slot sizes 513 to 4096 train with dense gradients")
row("row-grads-cand-table", T, train(tables(), batch(), cand(table=P, table_rows=100), pos(), flags=ROW_GRADS), INV, TRAIN_TABLE)
row("row-grads-null-dE", T, train(tables(), batch(), cand(), pos(), flags=ROW_GRADS, dE=None), INV, "null output")
row("row-grads-bias", T, train(tables(scorer=BIAS_E), batch(), cand(), pos(), flags=ROW_GRADS), UNS,
    "okge_train_forward_backward(OKGE_TRAIN_ROW_GRADS) does not take the OKGE_BIAS_ENTITY scorer: the unused slot's rows have no "
    "gradient to store")
row("row-grads-workspace", T, train(tables(), batch(), cand(), pos(), flags=ROW_GRADS, ws_bytes=16), WS,
    "workspace too small (okge_train_row_grads_workspace_bytes)")


# ---- the sharded phases -----------------------------------------------------------------------------------------------------
def tiles(t, sh, c, p, Q=P, ldq=64, B=4, flags=0, dQ=P, ws=P, ws_bytes=HUGE, norm=1.0):
    return (R(t), R(sh), Q, ldq, B, R(c), R(p), nv.OKGE_LOSS_BCE, 0.0, norm, 0, flags, None, P, P, dQ, ws, ws_bytes, None)


T = "okge_train_tiles"
row("tiles-bad-tables", T, tiles(None, shard(), cand(), pos()), INV, "bad tables")
row("tiles-null-cand", T, tiles(tables(), shard(), None, pos()), INV, "bad tables")
row("tiles-d-516", T, tiles(tables(d=516), shard(), cand(), pos()), UNS, D512_TRAIN_TILES)
row("tiles-null-shard", T, tiles(tables(), None, cand(), pos()), INV, "null shard descriptor")
row("tiles-shard-range", T, tiles(tables(), shard(0, 99), cand(), pos()), INV, SHARD_RANGE)
row("tiles-null-Q", T, tiles(tables(), shard(), cand(), pos(), Q=None), INV, "bad query block / candidates")
row("tiles-null-dQ", T, tiles(tables(), shard(), cand(), pos(), dQ=None), INV, "bad query block / candidates")
row("tiles-range", T, tiles(tables(), shard(), cand(first_id=60), pos()), INV, LOCAL_RANGE)
row("tiles-positives", T, tiles(tables(), shard(), cand(), None), INV, "bad positives")
row("tiles-normalizer", T, tiles(tables(), shard(), cand(), pos(), norm=-1.0), INV, "normalizer must be positive")
row("tiles-workspace", T, tiles(tables(), shard(), cand(), pos(), ws_bytes=16), WS, "workspace too small")
row("tiles-ldq", T, tiles(tables(), shard(), cand(), pos(), ldq=16), INV, "query block leading dimension must be okge_query_ld(d)")
row("tiles-clear-grads", T, tiles(tables(), shard(), cand(), pos(), flags=CLEAR_GRADS), INV, CLEAR_MSG)


def queries(t, sh, c, Q=P, ldq=64, B=4, scores=P, ld=64):
    return (R(t), R(sh), Q, ldq, B, R(c), scores, ld, None)


T = "okge_score_queries"
row("query-call-bad-tables", T, queries(tables(E=None), shard(), cand()), INV, "bad tables")
row("query-call-d-516", T, queries(tables(d=516), shard(), cand(), ldq=512), UNS, D512_QUERY_CALL)
row("query-call-null-shard", T, queries(tables(), None, cand()), INV, "null shard descriptor")
row("query-call-shard-range", T, queries(tables(), shard(5, 4), cand()), INV, SHARD_RANGE)
row("query-call-ldq", T, queries(tables(), shard(), cand(), ldq=16), INV, "bad query block / candidates")
row("query-call-no-rows", T, queries(tables(), shard(), cand(), B=0), INV, "bad query block / candidates")
row("query-call-cand-table", T, queries(tables(), shard(), cand(table=P, table_rows=100)), INV,
    "sharded calls take candidates from the local entity table")
row("query-call-range", T, queries(tables(), shard(), cand(first_id=-1)), INV, LOCAL_RANGE)
row("score-queries-scores", T, queries(tables(), shard(), cand(), scores=None), INV, "bad scores buffer")
row("row-lse-null-output", "okge_row_logsumexp", (R(tables()), R(shard()), P, 64, 4, R(cand()), None, P, HUGE, None), INV, "null output")
row("row-lse-workspace", "okge_row_logsumexp", (R(tables()), R(shard()), P, 64, 4, R(cand()), P, P, 16, None), WS, "workspace too small")
row("row-lse-range", "okge_row_logsumexp", (R(tables()), R(shard()), P, 64, 4, R(cand(first_id=51)), P, P, HUGE, None), INV, LOCAL_RANGE)

T = "okge_encode_queries"
row("encode-queries-common", T, (None, R(shard()), R(batch()), P, 64, None, None), INV, "null descriptor")
row("encode-queries-d-516", T, (R(tables(d=516)), R(shard()), R(batch()), P, 512, None, None), UNS, D512_TILE)
row("encode-queries-null-shard", T, (R(tables()), None, R(batch()), P, 64, None, None), INV, "null shard descriptor")
row("encode-queries-shard-range", T, (R(tables()), R(shard(-1, 99)), R(batch()), P, 64, None, None), INV, SHARD_RANGE)
row("encode-queries-no-output", T, (R(tables()), R(shard()), R(batch()), None, 64, None, None), INV, "bad query block")
row("encode-queries-ldq", T, (R(tables()), R(shard()), R(batch()), P, 16, None, None), INV, "bad query block")
T = "okge_fold_queries"
row("fold-queries-common", T, (R(tables()), R(batch(0, 0)), P, 64, P, None), INV, "empty batch")
row("fold-queries-bias", T, (R(tables(scorer=BIAS_R)), R(batch()), P, 64, P, None), UNS,
    "okge_fold_queries does not take the OKGE_BIAS_RELATION scorer: the sharded paths are not built for it")
row("fold-queries-null-rows", T, (R(tables()), R(batch()), None, 64, P, None), INV, "bad query block")
T = "okge_prefix_backward"
row("prefix-backward-common", T, (R(tables(d=4098)), R(shard()), R(batch()), P, 64, None, P, P, None), UNS,
    "slot sizes above 4096 are not supported")
row("prefix-backward-null-shard", T, (R(tables()), None, R(batch()), P, 64, None, P, P, None), INV, "null shard descriptor")
row("prefix-backward-null-dR", T, (R(tables()), R(shard()), R(batch()), P, 64, None, P, None, None), INV, "bad prefix_backward arguments")


def segmented(t, sh=None, dQ=P, ldq=64, rel=(P, P, 2), ent=(None, None, 0), grad_rows=P):
    return (R(t), R(sh or shard()), R(batch()), dQ, ldq, None) + rel + ent + (grad_rows, P, P, None)


T = "okge_prefix_backward_segmented"
SEG = "bad row segments (order[B], seg_ptr[n_seg + 1], 1 <= n_seg <= B; grad_rows[2][rows][ldq])"
row("segmented-common", T, segmented(tables(scorer=9)), INV, "unknown scorer")
row("segmented-shard-range", T, segmented(tables(), shard(0, 101)), INV, SHARD_RANGE)
row("segmented-null-dQ", T, segmented(tables(), dQ=None), INV, "bad prefix_backward arguments")
row("segmented-no-segments", T, segmented(tables(), rel=(None, None, 0)), INV, SEG)
row("segmented-null-seg-ptr", T, segmented(tables(), rel=(P, None, 2)), INV, SEG)
row("segmented-too-many", T, segmented(tables(), ent=(P, P, 5)), INV, SEG)
row("segmented-null-grad-rows", T, segmented(tables(), grad_rows=None), INV, SEG)
row("segmented-complex-d-12", T, segmented(tables(d=12)), UNS,
    "segmented gradients need d % 8 == 0 (ComplEx) / d % 4 == 0 (DistMult, data-bias)")
row("segmented-distmult-d-6", T, segmented(tables(d=6, scorer=nv.OKGE_DISTMULT)), UNS,
    "segmented gradients need d % 8 == 0 (ComplEx) / d % 4 == 0 (DistMult, data-bias)")


# ---- evaluation -------------------------------------------------------------------------------------------------------------
def ev_shard(t, sh, c, phase=1, Q=P, ldq=64, B=4, n_global=50, filt_ptr=P, n_filter=0, n_groups=3, ids=P, tru=P, ws=P, ws_bytes=HUGE):
    return (phase, R(t), R(sh), Q, ldq, B, R(c), n_global, filt_ptr, None, n_filter, P, P, ids, n_groups, tru, P, ws, ws_bytes, None)


T = "okge_evaluate_fused_shard"
row("eval-shard-phase", T, ev_shard(tables(), shard(), cand(), phase=3), INV, "phase must be 1 (points), 2 (sweep) or 4 (counts)")
row("eval-shard-null-tables", T, ev_shard(None, shard(), cand()), INV, "bad sharded evaluate arguments")
row("eval-shard-null-true", T, ev_shard(tables(), shard(), cand(), tru=None), INV, "bad sharded evaluate arguments")
row("eval-shard-bias", T, ev_shard(tables(scorer=BIAS_E), shard(), cand()), UNS,
    "okge_evaluate_fused_shard does not take the OKGE_BIAS_ENTITY scorer: the sharded paths are not built for it")
row("eval-shard-null-shard", T, ev_shard(tables(), None, cand()), INV, "null shard descriptor")
row("eval-shard-shard-range", T, ev_shard(tables(), shard(0, 50), cand()), INV, SHARD_RANGE)
row("eval-shard-ldq", T, ev_shard(tables(), shard(), cand(), ldq=16), INV, "query block leading dimension must be okge_query_ld(d)")
row("eval-shard-columns", T, ev_shard(tables(), shard(col0=10), cand()), INV,
    "the shard's candidate columns must lie inside the global candidate list")
row("eval-shard-range", T, ev_shard(tables(), shard(), cand(first_id=60), n_global=200), INV, LOCAL_RANGE)
row("eval-shard-arguments", T, ev_shard(tables(), shard(), cand(), filt_ptr=None), INV, "bad evaluate arguments")
row("eval-shard-null-ids", T, ev_shard(tables(), shard(), cand(), ids=None), INV, "bad evaluate arguments")
row("eval-shard-d-516", T, ev_shard(tables(d=516), shard(), cand(), ldq=512), UNS, D512_EVAL)
row("eval-shard-cand-table", T, ev_shard(tables(), shard(), cand(table=P, table_rows=100)), UNS, EVAL_MODE)
row("eval-shard-dropout", T, ev_shard(tables(), shard(), cand(drop=0.5)), UNS, EVAL_MODE)
row("eval-shard-workspace", T, ev_shard(tables(), shard(), cand(), ws_bytes=16), WS, "workspace too small")


def ev_fused(t, b, c, filt_ptr=P, n_filter=0, n_groups=3, ranks=P, ws=P, ws_bytes=HUGE):
    return (R(t), R(b), R(c), filt_ptr, None, n_filter, P, P, P, n_groups, ranks, P, ws, ws_bytes, None)


T = "okge_evaluate_fused"
row("eval-fused-common", T, ev_fused(tables(), batch(), cand(n=0)), INV, "no candidates")
row("eval-fused-d-516", T, ev_fused(tables(d=516), batch(), cand()), UNS, D512_TILE)
row("eval-fused-null-ranks", T, ev_fused(tables(), batch(), cand(), ranks=None), INV, "bad evaluate arguments")
row("eval-fused-filter", T, ev_fused(tables(), batch(), cand(), n_filter=2), INV, "bad evaluate arguments")
row("eval-fused-dropout", T, ev_fused(tables(), batch(drop=0.1), cand()), UNS, EVAL_MODE)
row("eval-fused-workspace", T, ev_fused(tables(), batch(), cand(), ws=None), WS, "workspace too small")
row("eval-batch-null-ranks", "okge_evaluate_batch",
    (R(tables()), R(batch()), R(cand()), P, None, P, P, P, 3, P, 64, None, P, P, HUGE, None, None), INV, "bad evaluate arguments")


def ev_batches(n_streams=2, streams=(P, P4), rank_offset=0, batches=True, c=None):
    eb = nv.EvalBatch(batch(), c or cand(), P, None, 0, P, P, P, 3, rank_offset)
    return (R(tables()), R(eb) if batches else None, 1, P, P, P, HUGE, arr(c_void_p, *streams), n_streams)


T = "okge_evaluate_fused_batches"
row("eval-batches-5-streams", T, ev_batches(5, (P, P4, P + 8, P + 12, P + 16)), INV, "bad evaluate arguments (1 to 4 streams)")
row("eval-batches-0-streams", T, ev_batches(0), INV, "bad evaluate arguments (1 to 4 streams)")
row("eval-batches-null-batches", T, ev_batches(batches=False), INV, "bad evaluate arguments (1 to 4 streams)")
row("eval-batches-equal-streams", T, ev_batches(2, (P, P)), INV, "okge_evaluate_fused_batches: the streams must differ")
row("eval-batches-rank-offset", T, ev_batches(rank_offset=-1), INV, "negative rank_offset")
row("eval-batches-eval-call", T, ev_batches(c=cand(drop=0.5)), UNS, EVAL_MODE)
row("filtered-ranks", "okge_filtered_ranks", (P, 49, 4, 50, P, P, P, P, P, P, None), INV, "bad rank arguments")
row("rank-metrics", "okge_rank_metrics", (None, 3, P, None), INV, "bad rank_metrics arguments")
row("group-true-scores", "okge_group_true_scores", (P, 64, 4, -1, 50, P, P, P, P, None), INV, "bad rank arguments")
row("rank-counts", "okge_rank_counts", (P, 64, 4, 0, 50, P, P, P, None, P, None), INV, "bad rank arguments")

# ---- encoders and row utilities ---------------------------------------------------------------------------------------------
T = "okge_score_triples"
row("triples-arguments", T, (0, None, 16, P, 16, P, 16, 3, 16, P, None), INV, "bad score_triples arguments")
row("triples-unknown-scorer", T, (8, P, 16, P, 16, P, 16, 3, 16, P, None), INV, "unknown scorer")
row("triples-bias", T, (BIAS_R, P, 16, P, 16, P, 16, 3, 16, P, None), UNS,
    "okge_score_triples does not take the OKGE_BIAS_RELATION scorer: it scores prefixes only (model.py:311-312, :347-348)")
row("triples-odd-complex", T, (0, P, 16, P, 16, P, 16, 3, 15, P, None), INV, "ComplEx needs an even slot size")
row("encode-rows-arguments", "okge_encode_rows", (P, 10, 8, None, 0, 3, None, P, 7, None), INV, "bad encode_rows arguments")
row("encode-rows-range", "okge_encode_rows", (P, 10, 8, None, 8, 3, None, P, 8, None), INV, "row range outside the table")
row("scatter-rows-arguments", "okge_scatter_rows", (None, 8, None, None, 0, 3, 8, None, P, 10, None), INV, "bad scatter_rows arguments")
row("scatter-rows-range", "okge_scatter_rows", (P, 8, None, None, 8, 3, 8, None, P, 10, None), INV, "row range outside the table")
row("scatter-rows-order", "okge_scatter_rows", (P, 8, P, None, 0, 3, 8, None, P, 10, None), INV,
    "scatter_rows with ids needs the positions sorted by id")


def psb(scorer=0, g=P, d=16, d_ent=P, ws=P, ws_bytes=HUGE):
    return (scorer, 0, g, 50, 4, 50, P, d, P, d, P, d, d, d_ent, P, P, ws, ws_bytes, None)


T = "okge_prefix_score_backward"
row("score-backward-arguments", T, psb(g=None), INV, "bad prefix_score_backward arguments")
row("score-backward-scorer", T, psb(scorer=4), INV, "unknown scorer")
row("score-backward-odd-complex", T, psb(d=15), INV, "ComplEx needs an even slot size")
row("score-backward-workspace", T, psb(ws_bytes=16), WS, "workspace too small or unaligned (okge_prefix_score_backward_workspace_bytes)")
row("score-backward-unaligned", T, psb(ws=P4), WS, "workspace too small or unaligned (okge_prefix_score_backward_workspace_bytes)")

T = "okge_tucker3_fold"
row("tucker3-fold-row-counts", T, (P, 8, 8, P, 8, P, 8, -1, 2, P, 64, P, HUGE, None), INV, "bad tucker3 arguments (row counts)")
row("tucker3-fold-null-W", T, (None, 8, 8, P, 8, P, 8, 2, 2, P, 64, P, HUGE, None), INV, "bad tucker3 arguments (W, d, r_e, rows)")
row("tucker3-fold-d-260", T, (P, 260, 8, P, 260, P, 8, 2, 2, P, 64, P, HUGE, None), UNS,
    "tucker3: slot sizes / relation sizes above 256 are not supported")
row("tucker3-fold-workspace", T, (P, 8, 8, P, 8, P, 8, 2, 2, P, 64, P, 16, None), WS, TUCKER_WS)
row("tucker3-fold-ldq", T, (P, 8, 8, P, 8, P, 8, 2, 2, P, 8, P, HUGE, None), INV,
    "bad tucker3_fold arguments (rows, query block: ldq = okge_query_ld(d))")
T = "okge_tucker3_backward"
row("tucker3-backward-row-counts", T, (P, 8, 8, P, 8, P, 8, P, 8, 2, -2, 0, P, P, P, P, HUGE, None), INV, "bad tucker3 arguments (row counts)")
row("tucker3-backward-unaligned", T, (P, 8, 8, P, 8, P, 8, P, 8, 2, 2, 0, P, P, P, P4, HUGE, None), WS, TUCKER_WS)
row("tucker3-backward-null-dQ", T, (P, 8, 8, P, 8, P, 8, None, 8, 2, 2, 0, P, P, P, P, HUGE, None), INV, "bad tucker3_backward arguments (rows, dQ)")
row("tucker3-backward-flags", T, (P, 8, 8, P, 8, P, 8, P, 8, 2, 2, 2, P, P, P, P, HUGE, None), INV, "tucker3_backward takes OKGE_TRAIN_GRADS_ZERO only")
T = "okge_tucker3_score_triples"
row("tucker3-triples-no-rows", T, (P, 8, 8, P, 8, P, 8, P, 8, 0, P, P, HUGE, None), INV, "bad tucker3 arguments (W, d, r_e, rows)")
row("tucker3-triples-arguments", T, (P, 8, 8, P, 8, P, 7, P, 8, 3, P, P, HUGE, None), INV, "bad tucker3_score_triples arguments")
row("tucker3-apply-arguments", "okge_tucker3_apply", (P, 63, P, 8, 3, 8, 0, P, 8, None), INV, "bad tucker3_apply arguments")
row("tucker3-apply-d-260", "okge_tucker3_apply", (P, 260 * 260, P, 260, 3, 260, 0, P, 260, None), UNS,
    "tucker3: slot sizes above 256 are not supported")
row("tucker3-outer-arguments", "okge_tucker3_outer", (P, 8, None, 8, 3, 8, P, 64, None), INV, "bad tucker3_outer arguments")
row("tucker3-outer-d-260", "okge_tucker3_outer", (P, 260, P, 260, 3, 260, P, 260 * 260, None), UNS,
    "tucker3: slot sizes above 256 are not supported")


# ---- token-pooled embedder --------------------------------------------------------------------------------------------------
def pool_encode(e, first_id=0, n=5):
    return (R(e), None, first_id, n, 0, P, P + 1024, 8, None, None, 0, None)


T = "okge_pool_encode"
row("embedder-null", T, pool_encode(None), INV, "bad token embedder")
row("embedder-null-W", T, pool_encode(embedder(W=None)), INV, "bad token embedder")
row("embedder-pool-3", T, pool_encode(embedder(pool=3)), INV, "pool must be 0 (sum), 1 (mean) or 2 (max)")
row("embedder-max-len-65", T, pool_encode(embedder(max_len=65)), UNS, "token sequences longer than 64 are not supported")
row("embedder-range", T, pool_encode(embedder(), first_id=28), INV, "row range outside the token-id table")
row("embedder-negative-n", T, pool_encode(embedder(), n=-1), INV, "row range outside the token-id table")
row("embedder-batch-norm", T, pool_encode(embedder(bn_weight=P)), INV, "batch-norm needs weight, bias and running statistics")
row("pool-backward-embedder", "okge_pool_backward", (None, None, 0, 5, P, P, 8, None, P, None, None, None, 0, None), INV, "bad token embedder")


def pool_calls(*calls, n_calls=None, training=1, ws=None, ws_bytes=0):
    return (arr(nv.PoolCall, *calls), len(calls) if n_calls is None else n_calls, training, ws, ws_bytes, None)


E0, EB = embedder(), embedder(bn=True)
T = "okge_pool_encode_calls"
row("pool-encode-0-calls", T, pool_calls(pool_call(E0), n_calls=0), INV, POOL_1_8)
row("pool-encode-9-calls", T, pool_calls(pool_call(E0), n_calls=9), INV, POOL_1_8)
row("pool-encode-null-calls", T, (None, 1, 1, None, 0, None), INV, POOL_1_8)
row("pool-call-embedder", T, pool_calls(pool_call(E0), pool_call(embedder(vocab=0))), INV, "bad token embedder")
row("pool-call-empty", T, pool_calls(pool_call(E0, n=0)), INV, "a pooled call needs n > 0 (leave empty calls out of the batch)")
row("pool-call-null-raw", T, pool_calls(pool_call(E0, raw=None)), INV, "bad row block")
row("pool-call-short-ld", T, pool_calls(pool_call(E0, ld=7)), INV, "bad row block")
row("pool-call-null-out", T, pool_calls(pool_call(E0, out=None)), INV, "bad output rows")
row("pool-call-bn-in-place", T, pool_calls(pool_call(EB, out=P)), INV,
    "with batch-norm the raw pooled rows are kept for backward: out must differ from raw")
row("pool-call-bn-no-saved", T, pool_calls(pool_call(EB)), INV, "training-mode batch-norm needs the saved-statistics buffer (4*d floats)")
row("pool-call-workspace", T, pool_calls(pool_call(EB, saved=P)), WS, "workspace too small (sum of okge_pool_workspace_bytes over the calls)")
row("pool-call-short-workspace", T, pool_calls(pool_call(EB, saved=P), ws=P, ws_bytes=16), WS,
    "workspace too small (sum of okge_pool_workspace_bytes over the calls)")


def pool_bwd(*calls, n_calls=None, ws=P, ws_bytes=HUGE, state=None, state_bytes=0):
    return (arr(nv.PoolCall, *calls), len(calls) if n_calls is None else n_calls, ws, ws_bytes, state, state_bytes, None)


T = "okge_pool_backward_calls"
row("pool-backward-0-calls", T, pool_bwd(pool_call(E0), n_calls=0), INV, POOL_1_8)
row("pool-backward-null-d-out", T, pool_bwd(pool_call(E0, dW=P)), INV, "bad backward arguments")
row("pool-backward-bn", T, pool_bwd(pool_call(EB, d_out=P, dW=P, saved=P)), INV,
    "batch-norm backward needs saved statistics and gradient buffers")
row("pool-backward-stamp", T, pool_bwd(pool_call(E0, d_out=P, dW=P, row_touched=P, touched_stamp=256)), INV, STAMP)
row("pool-backward-scatter-max-pool", T, pool_bwd(pool_call(embedder(pool=2), d_out=P, dW=P), state=P, state_bytes=HUGE), UNS,
    "the scatter plan needs sum / mean pooling, slot sizes that are a multiple of 4 and calls of one token table to agree in token "
    "matrix and touched map (pass scatter_state = NULL)")
row("pool-backward-scatter-state", T, pool_bwd(pool_call(E0, d_out=P, dW=P), state=P, state_bytes=16), WS,
    "scatter state too small (okge_pool_scatter_state_bytes)")
row("pool-backward-scatter-workspace", T, pool_bwd(pool_call(E0, d_out=P, dW=P), ws_bytes=16, state=P, state_bytes=HUGE), WS,
    "workspace too small (okge_pool_backward_workspace_bytes)")
row("pool-backward-scatter-alignment", T, pool_bwd(pool_call(E0, d_out=P, dW=P), state=P4, state_bytes=HUGE), INV,
    "scatter state and workspace must be 16-byte aligned")


def catch_up(call, table, n_calls=1, n_tables=1, counters=P):
    return (arr(nv.PoolCall, call), n_calls, arr(nv.LazyTensor, table), n_tables, counters, 0.1, 0.0, 1e-8, None)


T = "okge_pool_catch_up_calls"
row("catch-up-0-calls", T, catch_up(pool_call(E0), lazy_t(), n_calls=0), INV, POOL_1_8)
row("catch-up-5-tables", T, catch_up(pool_call(E0), lazy_t(), n_tables=5), INV, "bad catch-up arguments")
row("catch-up-null-counters", T, catch_up(pool_call(E0), lazy_t(), counters=None), INV, "bad catch-up arguments")
row("catch-up-embedder", T, catch_up(pool_call(embedder(pool=-1)), lazy_t()), INV, "pool must be 0 (sum), 1 (mean) or 2 (max)")
row("catch-up-empty-call", T, catch_up(pool_call(E0, n=0), lazy_t()), INV, "a pooled call needs n > 0 (leave empty calls out of the batch)")
row("catch-up-lazy-tensor", T, catch_up(pool_call(E0), lazy_t(steps=P, rows=20, row_len=6)), INV,
    "deferred rows need a row length that is a multiple of 4 and fewer than 2^31 rows")
row("catch-up-shape", T, catch_up(pool_call(E0), lazy_t(steps=P, rows=21, row_len=8)), INV, "lazy tensor and token table differ in shape")

# ---- optimizers and scaling -------------------------------------------------------------------------------------------------
row("adagrad-step-null", "okge_adagrad_step", (P, None, P, 16, 0.1, 0.0, 1e-8, 0, None), INV, "bad adagrad arguments")
row("adagrad-step-alignment", "okge_adagrad_step", (P, P, P4, 16, 0.1, 0.0, 1e-8, 0, None), INV, ALIGN16)
row("adagrad-step2-null", "okge_adagrad_step2", (P, P, P, 16, P, P, None, 16, 0.1, 0.0, 1e-8, 0, None), INV, "bad adagrad arguments")
row("adagrad-step2-negative-n", "okge_adagrad_step2", (P, P, P, 16, P, P, P, -1, 0.1, 0.0, 1e-8, 0, None), INV, "bad adagrad arguments")
row("adagrad-step2-alignment", "okge_adagrad_step2", (P, P, P, 16, P, P4, P, 16, 0.1, 0.0, 1e-8, 0, None), INV, ALIGN16)


def multi(*ts, n=None):
    return (arr(nv.AdagradTensor, *ts), len(ts) if n is None else n, 0.1, 0.0, 1e-8, None)


T = "okge_adagrad_multi"
row("adagrad-multi-0-tensors", T, multi(adagrad_t(), n=0), INV, "1 to 4 tensors per adagrad launch")
row("adagrad-multi-5-tensors", T, multi(adagrad_t(), n=5), INV, "1 to 4 tensors per adagrad launch")
row("adagrad-multi-null", T, multi(adagrad_t(), adagrad_t(s=None)), INV, "bad adagrad arguments")
row("adagrad-multi-alignment", T, multi(adagrad_t(p=P4)), INV, ALIGN16)
row("adagrad-multi-touched-rows", T, multi(adagrad_t(touched=P, row_len=3, stamp=1, zero_grad=1)), INV,
    "a touched-row map needs rows of a multiple of 4 floats that tile the tensor")
row("adagrad-multi-touched-tiling", T, multi(adagrad_t(n=18, touched=P, row_len=4, stamp=1, zero_grad=1)), INV,
    "a touched-row map needs rows of a multiple of 4 floats that tile the tensor")
row("adagrad-multi-stamp", T, multi(adagrad_t(touched=P, row_len=4, stamp=0, zero_grad=1)), INV, STAMP)
row("adagrad-multi-zero-grad", T, multi(adagrad_t(touched=P, row_len=4, stamp=1, zero_grad=0)), INV,
    "a touched-row map needs zero_grad (rows not stamped must hold zero gradients)")


def lazy(*ts, n=None, counters=P, window=4, mode=0):
    return (arr(nv.LazyTensor, *ts), len(ts) if n is None else n, counters, window, mode, 0.1, 0.0, 1e-8, None)


T = "okge_adagrad_lazy"
LAZY_ARGS = "okge_adagrad_lazy needs the counters, window >= 1 and mode OKGE_LAZY_STEP / OKGE_LAZY_FLUSH"
row("lazy-0-tensors", T, lazy(lazy_t(), n=0), INV, "1 to 4 tensors per adagrad launch")
row("lazy-null-counters", T, lazy(lazy_t(), counters=None), INV, LAZY_ARGS)
row("lazy-window-0", T, lazy(lazy_t(), window=0), INV, LAZY_ARGS)
row("lazy-mode-2", T, lazy(lazy_t(), mode=2), INV, LAZY_ARGS)
row("lazy-null-tensor", T, lazy(lazy_t(g=None)), INV, "bad lazy adagrad tensor")
row("lazy-row-len", T, lazy(lazy_t(steps=P, row_len=6)), INV,
    "deferred rows need a row length that is a multiple of 4 and fewer than 2^31 rows")
row("lazy-alignment", T, lazy(lazy_t(steps=P, s=P4)), INV, ALIGN16)
row("lazy-stamp", T, lazy(lazy_t(steps=P, touched=P, stamp=0)), INV, STAMP)
row("lazy-touched-without-steps", T, lazy(lazy_t(touched=P, stamp=1)), INV, "a touched-row map needs row_steps")


def rows(*ts, n=None, ws=P, ws_bytes=HUGE):
    return (arr(nv.RowsTensor, *ts), len(ts) if n is None else n, 0.1, 1e-8, ws, ws_bytes, None)


T = "okge_adagrad_rows"
row("rows-3-tensors", T, rows(rows_t(), n=3), INV, "one or two tensors")
row("rows-negative-n", T, rows(rows_t(n=-1)), INV, "negative occurrence count")
row("rows-too-many", T, rows(rows_t(n=(1 << 20) + 1)), UNS, "okge_adagrad_rows takes up to 2^20 occurrence rows per tensor")
row("rows-null-tensor", T, rows(rows_t(ids=None)), INV, "null tensor")
row("rows-shape", T, rows(rows_t(ld_g=3)), INV, "bad table shape / leading dimension")
row("rows-workspace", T, rows(rows_t(), ws_bytes=16), WS, ROWS_WS)


def catch_rows(*ts, n=None, counters=P):
    return (arr(nv.RowsDecayTensor, *ts), len(ts) if n is None else n, counters, 0.1, 0.0, 1e-8, None)


T = "okge_rows_catch_up"
row("rows-catch-up-3-tensors", T, catch_rows(decay_t(), n=3), INV, "one or two tensors")
row("rows-catch-up-counters", T, catch_rows(decay_t(), counters=None), INV, "okge_rows_catch_up needs the counters")
row("rows-catch-up-negative-n", T, catch_rows(decay_t(n=-1)), INV, "negative occurrence count")
row("rows-catch-up-too-many", T, catch_rows(decay_t(n=(1 << 20) + 1)), UNS, "okge_rows_catch_up takes up to 2^20 occurrence rows per tensor")
row("rows-catch-up-null-steps", T, catch_rows(decay_t(steps=None)), INV, "null tensor / bad table shape")
row("rows-catch-up-null-ids", T, catch_rows(decay_t(ids=None)), INV, "null ids")
row("rows-catch-up-row-len", T, catch_rows(decay_t(row_len=6, ld_g=6)), UNS,
    "deferred weight decay needs row_len % 4 == 0 and 16-byte aligned tables")
row("rows-catch-up-alignment", T, catch_rows(decay_t(p=P4)), UNS, "deferred weight decay needs row_len % 4 == 0 and 16-byte aligned tables")


def decay_rows(*ts, n=None, counters=P, window=4, ws=P, ws_bytes=HUGE):
    return (arr(nv.RowsDecayTensor, *ts), len(ts) if n is None else n, counters, window, 0.1, 0.0, 1e-8, ws, ws_bytes, None)


T = "okge_adagrad_rows_decay"
row("rows-decay-0-tensors", T, decay_rows(decay_t(), n=0), INV, "one or two tensors")
row("rows-decay-window", T, decay_rows(decay_t(), window=0), INV, "okge_adagrad_rows_decay needs the counters and window >= 1")
row("rows-decay-too-many", T, decay_rows(decay_t(n=(1 << 20) + 1)), UNS, "okge_adagrad_rows_decay takes up to 2^20 occurrence rows per tensor")
row("rows-decay-null-gradient", T, decay_rows(decay_t(g=None)), INV, "null gradient rows / bad leading dimension")
row("rows-decay-ld-g", T, decay_rows(decay_t(ld_g=6)), UNS, "deferred weight decay needs ld_g % 4 == 0 and 16-byte aligned gradient rows")
row("rows-decay-gradient-alignment", T, decay_rows(decay_t(g=P4)), UNS,
    "deferred weight decay needs ld_g % 4 == 0 and 16-byte aligned gradient rows")
row("rows-decay-workspace", T, decay_rows(decay_t(), ws=None), WS, ROWS_WS)
row("scale", "okge_scale_inplace", (P, 4, None, None), INV, "bad scale arguments")
row("rescale", "okge_rescale_gradients", (P, 4, None, 4, P, 1.0, None), INV, "bad rescale arguments")
row("rescale-applied-0", "okge_rescale_gradients", (P, 4, P, 4, P, 0.0, None), INV, "bad rescale arguments")
row("clip-arguments", "okge_clip_grad_norm", (P, 4, P, 4, 0.0, P, P, HUGE, None), INV, "bad clip_grad_norm arguments")
row("clip-workspace", "okge_clip_grad_norm", (P, 4, P, 4, 1.0, P, P, 8447, None), WS, "workspace too small (8448 bytes)")
row("merge-lse", "okge_merge_logsumexp", (P, 0, 4, P, None), INV, "bad merge_logsumexp arguments")


@pytest.fixture(scope="module")
def L():
    if nv.needs_build():
        nv.build_native()
    return nv.lib()


@pytest.mark.parametrize("fn,args,rc,msg", ROWS)
def test_refusal(L, fn, args, rc, msg):
    assert getattr(L, fn)(*args) == rc
    assert L.okge_last_error().decode() == msg


def test_row_ids_are_unique():
    ids = [p.id for p in ROWS]
    assert len(ids) == len(set(ids))
