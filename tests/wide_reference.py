"""A plain numpy / torch-CPU restatement of okge_train_forward_backward at slot sizes 513 .. 4096 (csrc/okge_wide.hip +
wide_core in csrc/okge_api_train.hip).  Not a conftest: the tests import it.

Two restatements of one step on fp32 inputs:
  truth      float64 through oracle.kge_oracle.step_forward_backward (masks from dropout_keep_mask or given explicitly)
  yardstick  float32 "as a correct kernel computes", the calibration of the band rule (lstm_reference.band_check):
               masked rows     table[id] * (keep ? fp32(1) / (fp32(1) - fp32(p)) : 0)
               fold            every product and every sum rounded on its own (score_backward_reference.fold)
               scores          ONE sequential fp32 chain over d per score (score_backward_reference.chain)
               loss, G         the oracle's formulas in fp32, G = g / fp32(normalizer)
               dC = G^T . Q    one chain over the batch rows (product_dc), times the mask, added to dE
               dQ = G . Cm     per candidate range of plan(): the range's candidates cut into dq_splits pieces of dq_k_per,
                               one chain each, the slabs added in split order; later ranges add to the earlier sum
               fold backward   plain fp32, times the masks, added to dE / dR
plan() restates okge_plan.h's plan_wide (tests/test_wide_plan.py pins the two against each other through the library's
workspace sizes; test_wide_reference.py pins this file's numbers against the driver)."""
import numpy as np

import score_backward_reference as sbr
from oracle import kge_oracle as ko

TM = TN = 128
GEMM_TILE, GEMM_K = 64, 16
STREAMS = dict(cand=0, po_ent=1, po_rel=2, sp_ent=3, sp_rel=4)        # hotpath.STREAM_*


def plan(B, N, d, gt_mbytes=None):
    """dict(Bpad, ldq, tiles, range_tiles, n_ranges, range_n, dq_splits, dq_k_per) as plan_wide answers"""
    Bpad, ldq, tiles = -(-B // TM) * TM, -(-d // 16) * 16, -(-N // TN)
    budget = max(1, 1024 if gt_mbytes is None else gt_mbytes) << 20
    rt = max(1, min(budget // (TN * (Bpad + 2 * ldq) * 4), tiles))
    n_ranges = -(-tiles // rt)
    rt = -(-tiles // n_ranges)
    n_ranges = -(-tiles // rt)
    range_n = rt * TN
    out_tiles = -(-B // GEMM_TILE) * -(-d // GEMM_TILE)
    kn = min(range_n, N)
    splits = max(1, min(64, 1024 // out_tiles, (kn + 4 * GEMM_K - 1) // (4 * GEMM_K)))
    k_per = -(-(-(-kn // splits)) // GEMM_K) * GEMM_K
    return dict(Bpad=Bpad, ldq=ldq, tiles=tiles, range_tiles=rt, n_ranges=n_ranges, range_n=range_n,
                dq_splits=-(-kn // k_per), dq_k_per=k_per)


def philox_masks(seed, step, n_po, n_sp, n_cand, d, p_ent, p_rel):
    """the five keep masks of one step as the kernels draw them (row key = position in its list)"""
    km = lambda name, n, p: ko.dropout_keep_mask(seed, STREAMS[name], step, n, d, p) if (n and p > 0) else None   # noqa: E731
    return dict(keep_cand=km("cand", n_cand, p_ent), keep_po_ent=km("po_ent", n_po, p_ent), keep_po_rel=km("po_rel", n_po, p_rel),
                keep_sp_ent=km("sp_ent", n_sp, p_ent), keep_sp_rel=km("sp_rel", n_sp, p_rel))


def _parts(z):
    po = (z["po_rel"].reshape(-1), z["po_obj"].reshape(-1)) if "po_rel" in z and len(z["po_rel"]) else None
    sp = (z["sp_subj"].reshape(-1), z["sp_rel"].reshape(-1)) if "sp_subj" in z and len(z["sp_subj"]) else None
    return po, sp


def truth(scorer, E, R, z, cand, y, loss="bce", smoothing=0.0, p_ent=0.0, p_rel=0.0, masks=None):
    """the step in float64: dict(loss, outputs, dE, dR, ...)"""
    po, sp = _parts(z)
    masks = masks or {}
    return ko.step_forward_backward(ko.KIND_NAMES[scorer], np.asarray(E, np.float64), np.asarray(R, np.float64), po, sp, cand,
                                    np.asarray(y, np.float64), ko.LOSS_NAMES[loss], smoothing, p_ent=p_ent, p_rel=p_rel,
                                    **{k: v for k, v in masks.items() if v is not None})


def _masked(table, ids, keep, p):
    rows = np.asarray(table, np.float32)[np.asarray(ids, np.int64)]
    return rows, (None if keep is None or p <= 0 else sbr.drop_mult(keep, p))


def yardstick(scorer, E, R, z, cand, y, loss="bce", smoothing=0.0, p_ent=0.0, p_rel=0.0, masks=None, gt_mbytes=None, dE0=None, dR0=None):
    """the step in float32 as a correct kernel computes it (see the module text): dict(loss, outputs, dE, dR, G, Q)"""
    f32 = np.float32
    E, R, cand = np.asarray(E, f32), np.asarray(R, f32), np.asarray(cand, np.int64).reshape(-1)
    masks = masks or {}
    po, sp = _parts(z)
    C, mc = _masked(E, cand, masks.get("keep_cand"), p_ent)
    Cm = C if mc is None else C * mc
    rows = []                                                      # (sp?, masked ent, masked rel, ent ids, rel ids, mult ent, mult rel)
    if po is not None:
        e, me = _masked(E, po[1], masks.get("keep_po_ent"), p_ent)
        r, mr = _masked(R, po[0], masks.get("keep_po_rel"), p_rel)
        rows.append((False, e if me is None else e * me, r if mr is None else r * mr, po[1], po[0], me, mr))
    if sp is not None:
        e, me = _masked(E, sp[0], masks.get("keep_sp_ent"), p_ent)
        r, mr = _masked(R, sp[1], masks.get("keep_sp_rel"), p_rel)
        rows.append((True, e if me is None else e * me, r if mr is None else r * mr, sp[0], sp[1], me, mr))
    Q = np.concatenate([sbr.fold(scorer, s, e, r, f32) for (s, e, r, *_x) in rows], axis=0)
    X = sbr.chain(Q, np.ascontiguousarray(Cm.T))
    B, N = X.shape
    d = E.shape[1]
    lsum, g = ko.loss_and_dscore(X, np.asarray(y, f32), ko.LOSS_NAMES[loss], smoothing)
    G = (g / f32(B * N)).astype(f32)
    pl = plan(B, N, d, gt_mbytes)
    dC = sbr.product_dc(G, Q, f32)
    dQ = np.zeros((B, d), f32)
    for r in range(pl["n_ranges"]):
        lo, hi = r * pl["range_n"], min(N, (r + 1) * pl["range_n"])
        for s in range(pl["dq_splits"]):
            k0, k1 = lo + s * pl["dq_k_per"], min(hi, lo + (s + 1) * pl["dq_k_per"])
            if k1 > k0:
                dQ = dQ + sbr.chain(G[:, k0:k1], Cm[k0:k1])
    dE = np.zeros_like(E) if dE0 is None else np.asarray(dE0, f32).copy()
    dR = np.zeros_like(R) if dR0 is None else np.asarray(dR0, f32).copy()
    np.add.at(dE, cand, dC if mc is None else dC * mc)
    b = 0
    for (s, e, r, e_ids, r_ids, me, mr) in rows:
        n = e.shape[0]
        de, dr = sbr.fold_backward(scorer, s, e, r, dQ[b:b + n], f32)
        np.add.at(dE, np.asarray(e_ids, np.int64), de if me is None else de * me)
        np.add.at(dR, np.asarray(r_ids, np.int64), dr if mr is None else dr * mr)
        b += n
    return dict(loss=float(lsum), outputs=X, dE=dE, dR=dR, G=G, Q=Q, dQ=dQ)
