"""A float64 restatement of the two data-bias scorers (DataBiasOnlyRelationScorer / DataBiasOnlyEntityScorer,
openkge/model.py:281-350) -- fold, prefix scores, chain rule -- and of one training step of DataBiasOnly{Entity,Relation}Model
composed with the LSTM pass of tests/lstm_reference.py.  Not a conftest: the tests import it.

    fold:        q = rel (bias_relation) | ent (bias_entity), ent = the prefix entity row (po: the object, sp: the subject)
    scores:      q . cand^T
    chain rule:  the used operand's gradient is dq; the other operand has NO gradient (None, not zeros: the reference's
                 autograd never reaches it, torch optimizers skip it)
"""
import numpy as np
import torch

from lstm_reference import GRAD_NAMES, lstm_pass

SIDES = ("entity", "relation")
LSTM_KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
SCORER_OF = {"DataBiasOnlyRelationModel": "bias_relation", "DataBiasOnlyEntityModel": "bias_entity"}


def fold(scorer, ent, rel):
    return {"bias_relation": rel, "bias_entity": ent}[scorer]


def scores(scorer, ent, rel, cand):
    return fold(scorer, ent, rel) @ cand.T


def chain(scorer, dq):
    """-> (d_ent, d_rel); None where the operand does not reach the score"""
    return (None, dq) if scorer == "bias_relation" else (dq, None)


def slot_params(params, side):
    """fixture name -> array map -> (W, lstm tensors, bn or None) of one slot, torch float32"""
    p = lambda k: torch.from_numpy(np.asarray(params[f"{side}_{k}"]))     # noqa: E731
    bn = (p("batchnorm.weight"), p("batchnorm.bias")) if f"{side}_batchnorm.weight" in params else None
    return p("embedding.weight"), [p(f"encoder_in.{k}") for k in LSTM_KEYS], bn


def grad_names(side, has_bn):
    names = [f"{side}_embedding.weight"] + [f"{side}_encoder_in.{k}" for k in LSTM_KEYS]
    return names + ([f"{side}_batchnorm.weight", f"{side}_batchnorm.bias"] if has_bn else [])


def step(scorer, params, bufs, tokens, batch, labels, normalizer):
    """One AddLossModule forward + (loss / normalizer).backward() in training mode (trainer.py:64-111): params / bufs map the
    fixture's names to arrays (bufs: running statistics, None = fresh), tokens = (ent_tokens, rel_tokens), batch = dict with
    cand, po_rel, po_obj and optionally sp_subj, sp_rel.  BCE-with-logits, reduction sum.  Returns loss, outputs, grads (name
    -> float64 array), grad_none (names), running (name -> array)."""
    ids = lambda k: torch.from_numpy(np.asarray(batch[k]).reshape(-1).astype(np.int64))      # noqa: E731
    has_sp = "sp_subj" in batch and batch["sp_subj"] is not None
    ent_calls = [ids("cand"), ids("po_obj")] + ([ids("sp_subj")] if has_sp else [])
    rel_calls = [ids("po_rel")] + ([ids("sp_rel")] if has_sp else [])
    n_c, n_po = ent_calls[0].numel(), ent_calls[1].numel()
    slots = {side: slot_params(params, side) for side in SIDES}

    def run(side, calls, d_out=None):
        W, lstm, bn = slots[side]
        running = None
        if bn is not None and bufs is not None:
            running = (torch.from_numpy(np.asarray(bufs[f"{side}_batchnorm.running_mean"])),
                       torch.from_numpy(np.asarray(bufs[f"{side}_batchnorm.running_var"])))
        return lstm_pass(W, torch.from_numpy(np.asarray(tokens[side == "relation"])), lstm, [(x, 0, x.numel()) for x in calls],
                         bn=bn, running=running, training=True, d_out=d_out)
    fe, fr = run("entity", ent_calls), run("relation", rel_calls)
    EV, RV = fe["out"], fr["out"]
    cand, ent, rel = EV[:n_c], EV[n_c:], RV                       # prefix rows: po first, then sp, in both tables
    x = scores(scorer, ent, rel, cand)
    y = np.asarray(labels, dtype=np.float64)
    loss = float((np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))).sum())
    G = (1.0 / (1.0 + np.exp(-x)) - y) / float(normalizer)
    d_cand, dq = G.T @ fold(scorer, ent, rel), G @ cand
    d_ent, d_rel = chain(scorer, dq)
    dEV = np.concatenate([d_cand, d_ent if d_ent is not None else np.zeros_like(ent)])
    res = {"loss": loss, "outputs": x, "grads": {}, "grad_none": [], "running": {}}
    for side, calls, d_out in (("entity", ent_calls, dEV), ("relation", rel_calls, d_rel)):
        has_bn = slots[side][2] is not None
        names = grad_names(side, has_bn)
        if d_out is None:                                          # the slot never reaches the score
            res["grad_none"] += names
            back = fr if side == "relation" else fe
        else:
            back = run(side, calls, torch.from_numpy(d_out))
            for name, k in zip(names, GRAD_NAMES):
                res["grads"][name] = back[k]
        if has_bn:
            res["running"][f"{side}_batchnorm.running_mean"] = back["running_mean"]
            res["running"][f"{side}_batchnorm.running_var"] = back["running_var"]
    _ = n_po
    return res


def adagrad(p, g, s, lr, weight_decay, eps):
    """torch.optim.Adagrad's dense update (lr_decay 0): -> (p, sum) after the step, float64"""
    p, s = np.asarray(p, np.float64), np.asarray(s, np.float64)
    g = np.asarray(g, np.float64) + weight_decay * p
    s = s + g * g
    return p - lr * g / (np.sqrt(s) + eps), s
