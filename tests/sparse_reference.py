"""NumPy statement of the row-sparse training step (include/okge.h: OKGE_TRAIN_ROW_GRADS, okge_adagrad_rows).

Occurrence-row layout: the entity gradient of one batch is (N + B, d) -- row j < N belongs to candidate column j, row N + i to
the prefix entity of batch row i (po rows first) -- and the relation gradient is (B, d), row i for batch row i.  The table row
each occurrence row belongs to is ids_e = [candidate ids | po_obj | sp_subj], ids_r = [po_rel | sp_rel].
Coalescing: per distinct id the occurrence rows are added in ascending position, sequentially in fp32.
Update: the oracle's dense Adagrad arithmetic at weight_decay = 0, on the touched rows only.
"""
import numpy as np

from oracle import kge_oracle as ko


def occurrence_ids(cand_ids, po, sp):
    """po = (rel_ids, obj_ids) or None, sp = (subj_ids, rel_ids) or None -> (ids_e, ids_r) int64"""
    flat = lambda a: np.asarray(a).reshape(-1).astype(np.int64)      # noqa: E731
    ent, rel = [flat(cand_ids)], []
    if po is not None and len(flat(po[0])):
        ent.append(flat(po[1]))
        rel.append(flat(po[0]))
    if sp is not None and len(flat(sp[0])):
        ent.append(flat(sp[0]))
        rel.append(flat(sp[1]))
    return np.concatenate(ent), np.concatenate(rel)


def row_grads(kind, E, R, po, sp, cand_ids, labels, **kw):
    """-> dict(loss, gE (N + B, d), gR (B, d), ids_e, ids_r): the oracle's step on the relabelled problem -- tables made of the
    occurrence rows, positions for ids -- whose dense gradients ARE the occurrence rows (every row is named once)"""
    ids_e, ids_r = occurrence_ids(cand_ids, po, sp)
    n = len(np.asarray(cand_ids).reshape(-1))
    n_po = 0 if po is None else len(np.asarray(po[0]).reshape(-1))
    n_sp = 0 if sp is None else len(np.asarray(sp[0]).reshape(-1))
    EV, RV = E[ids_e], R[ids_r]
    po_v = (np.arange(n_po), n + np.arange(n_po)) if n_po else None
    sp_v = (n + n_po + np.arange(n_sp), n_po + np.arange(n_sp)) if n_sp else None
    out = ko.step_forward_backward(kind, EV, RV, po_v, sp_v, np.arange(n), labels, **kw)
    return dict(loss=out["loss"], gE=out["dE"], gR=out["dR"], ids_e=ids_e, ids_r=ids_r)


def coalesce(ids, g, table_rows):
    """-> (dense (table_rows, d) gradient, touched (table_rows,) bool): per id ((g_a + g_b) + g_c) ... in ascending position,
    fp32; ids outside the table are skipped"""
    g = np.asarray(g, np.float32)
    dense = np.zeros((table_rows, g.shape[1]), np.float32)
    touched = np.zeros(table_rows, bool)
    for pos, i in enumerate(np.asarray(ids).reshape(-1)):
        if not 0 <= i < table_rows:
            continue
        dense[i] = dense[i] + g[pos] if touched[i] else g[pos]
        touched[i] = True
    return dense, touched


def adagrad_rows(p, state_sum, ids, g, lr, eps=1e-8):
    """in place, touched rows only: sum += g*g; p -= lr * g / (sqrt(sum) + eps) on the coalesced rows"""
    dense, touched = coalesce(ids, g, p.shape[0])
    rows = np.flatnonzero(touched)
    pr, sr = p[rows], state_sum[rows]
    ko.adagrad_step(pr, dense[rows], sr, lr, 0.0, eps)
    p[rows], state_sum[rows] = pr, sr
    return p, state_sum
