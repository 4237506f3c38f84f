"""NumPy restatement of the lookup embedder's `_encode` variants (openkge/model.py:455-480) and of its hand-written backward,
in any float dtype: the yardstick of csrc/okge_lookup_encode.hip and lookup_variants.LookupVariantTrainStep.  TEST
INFRASTRUCTURE, not product code.

A pass is the five encode calls of a batch in the reference's order (trainer.py:75-91): cand, po_rel, po_obj, sp_subj, sp_rel.
Per call: gather -> input dropout -> BatchNorm1d (oracle.kge_oracle.batchnorm_train / batchnorm_eval; bn_e for entity calls,
bn_r for relation calls; running statistics moved once per call, in call order) -> entity calls: rows . W^T (obj_projection
for cand and po_obj, subj_projection for sp_subj) [-> ReLU] -> F.normalize -> final dropout -> l2_reg hook.

P: dict of arrays E, R[, bn_e_w, bn_e_b, bn_e_mean, bn_e_var, bn_r_w, bn_r_b, bn_r_mean, bn_r_var][, W_subj, W_obj]
cfg: dict(batch_norm, project, activation ('ReLU' / None), normalize ('norm' / ''), l2_reg, dropout, relation_dropout,
     input_dropout, relation_input_dropout)
batch: dict of id arrays cand, po_rel, po_obj, sp_subj, sp_rel (None or empty: an empty call)
"""
import numpy as np

from oracle import kge_oracle as ko

CALLS = ("cand", "po_rel", "po_obj", "sp_subj", "sp_rel")
RELATION = (False, True, False, False, True)
INPUT_STREAMS = (16, 18, 17, 19, 20)               # include/okge.h OKGE_LOOKUP_STREAM_*, in CALLS order
FINAL_STREAMS = (0, 2, 1, 3, 4)                    # hotpath.STREAMS (cand, po_ent, po_rel, sp_ent, sp_rel), in CALLS order
NORM_EPS = 1e-12


def default_cfg(**kw):
    cfg = dict(batch_norm=False, project=False, activation="ReLU", normalize="", l2_reg=0.0, dropout=0.0, relation_dropout=0.0,
               input_dropout=0.0, relation_input_dropout=0.0)
    cfg.update(kw)
    return cfg


def cast(P, dt):
    return {k: np.asarray(v, dtype=dt).copy() for k, v in P.items()}


def _ids(batch, name):
    x = batch.get(name)
    return np.zeros(0, dtype=np.int64) if x is None else np.asarray(x).reshape(-1).astype(np.int64)


def philox_keeps(seed, step, d, batch, p_ent, p_rel, streams):
    """the five keep masks of one step (None where p == 0), keyed by the row's position in its call"""
    out = []
    for name, rel, stream in zip(CALLS, RELATION, streams):
        p, n = (p_rel if rel else p_ent), _ids(batch, name).size
        out.append(ko.dropout_keep_mask(seed, stream, step, n, d, p) if p > 0 and n else None)
    return out


def _mask(keep, p, dt):
    return keep.astype(dt) * (dt.type(1.0) / dt.type(1.0 - p))


def encode_pass(P, cfg, batch, dt, training=True, in_keeps=None):
    """-> (rows: the five calls' encoded rows in front of the final dropout, aux for backward_pass, running: the running
    statistics after the pass {bn_e_mean, ...}, min_var: the smallest batch variance any call normalised with)"""
    dt = np.dtype(dt)
    P = cast(P, dt)
    running = {k: P[k].copy() for k in P if k.endswith(("_mean", "_var"))}
    rows, aux, min_var = [], [], np.inf
    for i, (name, rel) in enumerate(zip(CALLS, RELATION)):
        ids = _ids(batch, name)
        a = dict(ids=ids, rel=rel)
        if ids.size == 0:
            rows.append(np.zeros((0, P["E"].shape[1]), dtype=dt))
            aux.append(a)
            continue
        x = P["R" if rel else "E"][ids]
        p_in = cfg["relation_input_dropout"] if rel else cfg["input_dropout"]
        if training and p_in > 0 and in_keeps is not None and in_keeps[i] is not None:
            a["in_mask"] = _mask(in_keeps[i], p_in, dt)
            x = x * a["in_mask"]
        if cfg["batch_norm"]:
            s = "bn_r" if rel else "bn_e"
            if training:
                if x.shape[0] == 1:
                    raise ValueError("Expected more than 1 value per channel when training")
                min_var = min(min_var, float(x.astype(np.float64).var(axis=0).min()))
                x, a["bn"] = ko.batchnorm_train(x, P[s + "_w"], P[s + "_b"], running[s + "_mean"], running[s + "_var"])
                x = x.astype(dt)
            else:
                x = ko.batchnorm_eval(x, P[s + "_w"], P[s + "_b"], P[s + "_mean"], P[s + "_var"]).astype(dt)
        if cfg["project"] and not rel:
            a["W"] = "W_subj" if name == "sp_subj" else "W_obj"
            a["xbn"] = x
            x = x @ P[a["W"]].T
            if cfg["activation"] == "ReLU":
                a["pos"] = x > 0
                x = np.where(a["pos"], x, dt.type(0))
        if cfg["normalize"] == "norm":
            nrm = np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), dt.type(NORM_EPS))
            x = x / nrm
            a["y"], a["nrm"] = x, nrm
        rows.append(x)
        aux.append(a)
    return rows, aux, running, min_var


def backward_pass(P, cfg, dt, aux, d_rows):
    """the exact chain rule of encode_pass (training mode): d_rows = the five calls' row gradients -> dict of parameter gradients
    E, R[, bn_e_w, bn_e_b, bn_r_w, bn_r_b][, W_subj, W_obj]; row 0 of a table (the padding row) receives nothing"""
    dt = np.dtype(dt)
    P = cast(P, dt)
    grads = {k: np.zeros_like(v) for k, v in P.items() if not k.endswith(("_mean", "_var"))}
    for a, g in zip(aux, d_rows):
        ids = a["ids"]
        if ids.size == 0:
            continue
        g = np.asarray(g, dtype=dt)
        if "y" in a:
            g = (g - a["y"] * (a["y"] * g).sum(axis=1, keepdims=True)) / a["nrm"]
        if "W" in a:
            if "pos" in a:
                g = np.where(a["pos"], g, dt.type(0))
            grads[a["W"]] += g.T @ a["xbn"]
            g = g @ P[a["W"]]
        if "bn" in a:
            s = "bn_r" if a["rel"] else "bn_e"
            g, dw, db = ko.batchnorm_train_backward(g, P[s + "_w"], a["bn"])
            grads[s + "_w"] += dw
            grads[s + "_b"] += db
        if "in_mask" in a:
            g = g * a["in_mask"]
        live = ids != 0
        np.add.at(grads["R" if a["rel"] else "E"], ids[live], g[live])
    return grads


def full_step(kind, P, cfg, batch, labels, dt, loss_kind=ko.LOSS_BCE, smoothing=0.0, normalizer=None, in_keeps=None, out_keeps=None,
              training=True):
    """AddLossModule.forward + `((loss + hook) / normalizer).backward()` (trainer.py:48-113, :217-222) over encode_pass with one
    shared candidate block.  -> dict(loss, hook, outputs, rows, grads, running, min_var)"""
    dt = np.dtype(dt)
    rows, aux, running, min_var = encode_pass(P, cfg, batch, dt, training, in_keeps)
    masks, dropped = [], []
    for i, (x, rel) in enumerate(zip(rows, RELATION)):
        p = cfg["relation_dropout"] if rel else cfg["dropout"]
        m = _mask(out_keeps[i], p, dt) if training and p > 0 and out_keeps is not None and out_keeps[i] is not None else None
        masks.append(m)
        dropped.append(x if m is None else x * m)
    cand, po_rel, po_obj, sp_subj, sp_rel = dropped
    n_po = po_rel.shape[0]
    Q = np.concatenate([ko.prefix_query(kind, ko.DIR_PO, po_obj, po_rel), ko.prefix_query(kind, ko.DIR_SP, sp_subj, sp_rel)], axis=0)
    X = Q @ cand.T
    B, N = X.shape
    if normalizer is None:
        normalizer = float(B * N)
    loss, g = ko.loss_and_dscore(X, np.asarray(labels, dtype=dt), loss_kind, smoothing)
    out = dict(loss=float(loss), hook=0.0, outputs=X, rows=rows, running=running, min_var=min_var)
    if not training:
        return out
    G = (g / dt.type(normalizer)).astype(dt)
    dQ, d_cand = G @ cand, G.T @ Q
    d_obj, d_po_rel = ko.prefix_query_backward(kind, ko.DIR_PO, po_obj, po_rel, dQ[:n_po])
    d_subj, d_sp_rel = ko.prefix_query_backward(kind, ko.DIR_SP, sp_subj, sp_rel, dQ[n_po:])
    d_rows = [d_cand, d_po_rel, d_obj, d_subj, d_sp_rel]
    if cfg["l2_reg"] > 0:                                            # model.py:471-479: rows / dropout (the probability) when > 0
        coef = cfg["l2_reg"] / cfg["dropout"] ** 3 if cfg["dropout"] > 0 else cfg["l2_reg"]
        hook = 0.0
        for i, x in enumerate(dropped):
            hook += coef * float((np.abs(x.astype(np.float64)) ** 3).sum())
            d_rows[i] = d_rows[i] + (dt.type(3.0 * coef / normalizer) * x * np.abs(x)).astype(dt)
        out["hook"] = hook
    d_rows = [g_ if m is None else g_ * m for g_, m in zip(d_rows, masks)]
    out["grads"] = backward_pass(P, cfg, dt, aux, d_rows)
    return out
