"""Float64 NumPy restatement of the reference's `l2_reg` hook (openkge/model.py:444-453, :471-479) as
okge_n3_forward_backward computes it (include/okge.h), for tests/test_n3_*.py.

Every _encode call in training mode adds  l2_reg * sum |x|^3  over the rows it returns; x is the row after both dropouts,
divided by `dropout` (the probability) when that is > 0; the Trainer backpropagates (loss + hook) / normalizer
(trainer.py:217-221).  With x = m s e -- m the keep flag, s = 1 / (1 - p) the scale of the ONE mask the fused path folds the
two dropouts into, e the stored element -- and c = l2_reg / dropout^3 (dropout > 0) or l2_reg:

    value      c * sum |x|^3
    d / d e    3 c x |x| m s / normalizer            (0 at x == 0)

The candidate block counts `passes` times (once with a shared list, once per direction present without one); a list that
repeats an id counts it as often as it is listed; every prefix entity row and every prefix relation row counts once per
occurrence.  s is the fp32 number the library multiplies by (okge.h, okge_dropout: "kept values are multiplied by 1/(1-p)",
formed in fp32), everything else is float64.
"""
import numpy as np

from oracle import kge_oracle as ko


def coef(l2_reg, dropout):
    return float(l2_reg) / float(dropout) ** 3 if dropout > 0 else float(l2_reg)


def mask_scale(p):
    """1 / (1 - p) as the library forms it: in fp32"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def rows_term(rows, keep, p, c, normalizer, passes=1):
    """(value, gradient rows) of `passes` encode calls returning rows * keep * s"""
    rows = np.asarray(rows, np.float64)
    s = mask_scale(p)
    m = np.ones_like(rows) if (keep is None or p <= 0) else np.asarray(keep).astype(np.float64)
    x = rows * m * s
    value = passes * c * (np.abs(x) ** 3).sum()
    grad = passes * 3.0 * c * x * np.abs(x) * m * s / normalizer
    return value, grad


def n3_term(E, R, po, sp, cand_ids, c, passes, normalizer, p_ent=0.0, p_rel=0.0, keep_cand=None, keep_po_ent=None,
            keep_sp_ent=None, keep_po_rel=None, keep_sp_rel=None):
    """-> dict(value, dE, dR: dense table gradients; gE (N + B, d), gR (B, d): the same in occurrence rows, candidates first,
    po rows before sp rows).  po = (rel_ids, obj_ids) or None, sp = (subj_ids, rel_ids) or None, as in the oracle."""
    E, R = np.asarray(E, np.float64), np.asarray(R, np.float64)
    ids = lambda a: np.asarray(a).reshape(-1).astype(np.int64)     # noqa: E731
    cand_ids = ids(cand_ids)
    value, gC = rows_term(E[cand_ids], keep_cand, p_ent, c, normalizer, passes)
    dE, dR = np.zeros_like(E), np.zeros_like(R)
    np.add.at(dE, cand_ids, gC)
    occ_e, occ_r = [gC], []
    for pair, ent_at, keep_e, keep_r in ((po, 1, keep_po_ent, keep_po_rel), (sp, 0, keep_sp_ent, keep_sp_rel)):
        if pair is None:
            continue
        e_ids, r_ids = ids(pair[ent_at]), ids(pair[1 - ent_at])
        ve, ge = rows_term(E[e_ids], keep_e, p_ent, c, normalizer)
        vr, gr = rows_term(R[r_ids], keep_r, p_rel, c, normalizer)
        value += ve + vr
        np.add.at(dE, e_ids, ge)
        np.add.at(dR, r_ids, gr)
        occ_e.append(ge)
        occ_r.append(gr)
    return dict(value=value, dE=dE, dR=dR, gE=np.concatenate(occ_e), gR=np.concatenate(occ_r))


def fixture_problem(z):
    """a g12_variant_l2 / g23_n3_* fixture -> the problem in one vocabulary"""
    g12 = "p0_entity_embedding.weight" in z.files
    f = dict(E=z["p0_entity_embedding.weight"] if g12 else z["E"], R=z["p0_relation_embedding.weight"] if g12 else z["R"],
             dE=z["g_entity_embedding.weight"] if g12 else z["dE"], dR=z["g_relation_embedding.weight"] if g12 else z["dR"],
             kind="complex" if g12 else str(z["model"]), cand=z["cand"].reshape(-1), labels=z["labels"], loss=float(z["loss"]),
             hook=float(z["hook"]), outputs=z["outputs"], normalizer=float(z["normalizer"]), l2_reg=float(z["l2_reg"]),
             no_shared="no_shared" in z.files and bool(z["no_shared"]), dropout=0.0 if g12 else float(z["dropout"]),
             input_dropout=0.0 if g12 else float(z["input_dropout"]))
    f["po"] = (z["po_rel"].reshape(-1), z["po_obj"].reshape(-1)) if "po_rel" in z.files else None
    f["sp"] = (z["sp_subj"].reshape(-1), z["sp_rel"].reshape(-1)) if "sp_subj" in z.files else None
    # the two dropouts of one _encode call as ONE mask: keep probability (1 - input_dropout)(1 - dropout) (model.py:461-470)
    f["p_ent"] = 1.0 - (1.0 - f["input_dropout"]) * (1.0 - f["dropout"])
    f["keeps"] = {k: z["mask_" + k[5:]] for k in ("keep_cand", "keep_po_ent", "keep_sp_ent") if "mask_" + k[5:] in z.files}
    f["passes"] = (int(f["po"] is not None) + int(f["sp"] is not None)) if f["no_shared"] else 1
    f["coef"] = coef(f["l2_reg"], f["dropout"])
    return f


def fixture_step(f):
    """the whole step of a fixture in float64: loss and outputs (the oracle), hook, gradient of (loss + hook) / normalizer"""
    E, R = f["E"].astype(np.float64), f["R"].astype(np.float64)
    step = ko.step_forward_backward(ko.KIND_NAMES[f["kind"]], E, R, f["po"], f["sp"], f["cand"], f["labels"].astype(np.float64),
                                    normalizer=f["normalizer"], p_ent=f["p_ent"], **f["keeps"])
    reg = n3_term(E, R, f["po"], f["sp"], f["cand"], f["coef"], f["passes"], f["normalizer"], p_ent=f["p_ent"], **f["keeps"])
    return dict(loss=step["loss"], outputs=step["outputs"], hook=reg["value"], dE=step["dE"] + reg["dE"], dR=step["dR"] + reg["dR"])
