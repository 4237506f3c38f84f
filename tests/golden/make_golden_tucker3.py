#!/usr/bin/env python3
"""Golden vectors for the Tucker3 lookup model (g18_tucker3_*), produced by running the REFERENCE itself on the CPU.

Run (never on the GPU box -- the reference is not there):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> \
        python3 -B <repo>/tests/golden/make_golden_tucker3.py <reference checkout>

The script imports the unmodified reference (openkge.model / openkge.trainer / utils.optim), drives
LookupTucker3RelationModel with small seeded inputs (d <= 16) and stores inputs and expected outputs as .npz fixtures next
to this file.  Fixtures are DATA only.

  g18_tucker3_<case>   the constructor's parameters for the seed ("ctor/"), the parameters the run uses ("init/": the
                       projection scaled so that the scores reach |x| ~ 3 -- with Xavier W and small tables they peak near
                       0.01, where an absolute tolerance would check nothing), batch, AddLossModule loss and outputs in
                       training mode, every parameter's gradient after (loss / normalizer).backward(), the Bernoulli
                       keep-masks the reference drew (dropout case), eval-mode sp / po prefix scores and triple scores.
  g18_tucker3_adagrad  three steps through the reference's OptimRegime Adagrad (lr 0.3, weight_decay 1e-10, leaked eps):
                       parameters and accumulators of all three tensors before the first and after every step.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("OKGE_REFERENCE", "")
assert REF and os.path.isdir(REF), "pass the reference checkout: golden vectors are made from the reference itself"
if REF not in sys.path:
    sys.path.insert(0, REF)

from openkge.dataset import EntityRelationDatasetMeta  # noqa: E402
from openkge.model import Models  # noqa: E402
from openkge.trainer import AddLossModule  # noqa: E402
from utils.optim import OptimRegime  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(4)
F = torch.nn.functional


def npy(t):
    return t.detach().cpu().numpy()


def save(name, **kw):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **kw)
    print("wrote", path, os.path.getsize(path), "bytes")


def dense_labels(rng, B, N, max_pos=4):
    y = np.zeros((B, N), dtype=np.float32)
    for b in range(B):
        y[b, rng.choice(N, size=int(rng.integers(1, max_pos + 1)), replace=False)] = 1.0
    return y


def rand_ids(rng, lo, hi, n):
    return torch.from_numpy(rng.integers(lo, hi, size=(n, 1)).astype(np.int32))


def build(seed, d, r_e, n_ent, n_rel, **model_kw):
    md = EntityRelationDatasetMeta(entity_id_count_map={}, relation_id_count_map={}, entity_token_id_count_map={},
                                   relation_token_id_count_map={}, entity_id_to_tokens_map=[], relation_id_to_tokens_map=[],
                                   entities_size=n_ent, relations_size=n_rel, min_entities_size=2, min_relations_size=2,
                                   entity_tokens_size=0, relation_tokens_size=0, max_length=(1, 1))
    torch.manual_seed(seed)
    m = Models.LookupTucker3RelationModel(entity_slot_size=d, relation_slot_size=r_e, train_data=md, init_std=0.3, sparse=False,
                                          **model_kw)
    kw = dict(seed=np.int64(seed), d=np.int64(d), r_e=np.int64(r_e), n_ent=np.int64(n_ent), n_rel=np.int64(n_rel), init_std=np.float64(0.3),
              param_names=np.array([k for k, _ in m.named_parameters()]), state_keys=np.array(list(m.state_dict().keys())))
    for k, p in m.named_parameters():
        kw["ctor/" + k] = npy(p).copy()
    # scale the projection so that the eval-mode scores of random prefixes peak near 3 (the score is linear in W)
    m.eval()
    with torch.no_grad():
        probe = np.random.default_rng(seed + 5)
        x = m.sp_prefix_score(rand_ids(probe, 2, n_ent, 16), rand_ids(probe, 2, n_rel, 16))
        m.relation_projection[0].weight.data.mul_(float(3.0 / x.abs().max()))
    m.train()
    for k, p in m.named_parameters():
        kw["init/" + k] = npy(p).copy()
    return m, kw


def batch(rng, n_ent, n_rel, b_po, b_sp, n_cand, repeat=False):
    if n_cand == "all":
        cand = torch.arange(n_ent)[2:].int().unsqueeze(1)
    else:
        ids = rng.permutation(np.arange(2, n_ent))[:n_cand].astype(np.int32)
        if repeat:
            ids[-1] = ids[3]                                   # an id twice in the batch-shared list
        cand = torch.from_numpy(ids).unsqueeze(1)
    po = (rand_ids(rng, 2, n_rel, b_po), rand_ids(rng, 2, n_ent, b_po)) if b_po else None
    sp = (rand_ids(rng, 2, n_ent, b_sp), rand_ids(rng, 2, n_rel, b_sp)) if b_sp else None
    return cand, po, sp, dense_labels(rng, b_po + b_sp, cand.shape[0])


def batch_kw(prefix, cand, po, sp, y):
    kw = {prefix + "cand": npy(cand), prefix + "labels": y}
    if po is not None:
        kw.update({prefix + "po_rel": npy(po[0]), prefix + "po_obj": npy(po[1])})
    if sp is not None:
        kw.update({prefix + "sp_subj": npy(sp[0]), prefix + "sp_rel": npy(sp[1])})
    return kw


def g18_cases():
    cases = [
        # name, d, r_e, n_ent, n_rel, b_po, b_sp, n_cand, repeat, loss, smoothing, input_dropout, relation_input_dropout
        ("bce_all", 12, 7, 66, 10, 6, 7, "all", False, "bce", 0.0, 0.0, 0.0),
        ("kl_shared", 16, 16, 80, 11, 7, 6, 40, True, "kl", 0.0, 0.0, 0.0),
        ("bce_smooth_po_only", 16, 5, 70, 9, 9, 0, "all", False, "bce", 0.1, 0.0, 0.0),
        ("bce_dropout", 12, 7, 66, 10, 6, 7, "all", False, "bce", 0.0, 0.4, 0.25),
    ]
    for ci, (name, d, r_e, n_ent, n_rel, b_po, b_sp, n_cand, repeat, loss, smoothing, p_in, p_rel) in enumerate(cases):
        seed = 1800 + ci
        rng = np.random.default_rng(seed)
        m, kw = build(seed, d, r_e, n_ent, n_rel, input_dropout=p_in, relation_input_dropout=p_rel, dropout=0.0, relation_dropout=0.0)
        cand, po, sp, y = batch(rng, n_ent, n_rel, b_po, b_sp, n_cand, repeat)
        B, N = y.shape
        lossf = torch.nn.BCEWithLogitsLoss(reduction="sum") if loss == "bce" else torch.nn.KLDivLoss(reduction="sum")
        mod = AddLossModule(m, lossf, bce_label_smoothing=smoothing)
        mod.train()
        if p_in > 0 or p_rel > 0:
            # Capture the Bernoulli keep-masks the reference is about to draw: same generator state, same op sequence
            # (candidates; po relations, po objects; sp subjects, sp relations -- trainer.py:75-91, model.py:52-74)
            st = torch.get_rng_state()
            torch.manual_seed(seed + 77)
            draw = lambda n, w, p: npy(F.dropout(torch.ones(n, w), p=p, training=True) > 0).astype(np.uint8)      # noqa: E731
            kw["mask_cand"] = draw(N, d, p_in)
            if b_po:
                kw["mask_po_rel"] = draw(b_po, r_e, p_rel)
                kw["mask_po_ent"] = draw(b_po, d, p_in)
            if b_sp:
                kw["mask_sp_ent"] = draw(b_sp, d, p_in)
                kw["mask_sp_rel"] = draw(b_sp, r_e, p_rel)
            torch.set_rng_state(st)
            torch.manual_seed(seed + 77)
        lval, hook, outputs = mod(inputs=[po, sp], labels=torch.from_numpy(y.copy()), use_batch_shared_entities=(n_cand != "all"),
                                  batch_shared_entities=cand, epoch=1, input_style_triple_or_prefix="right_and_left_prefix")
        assert hook is None
        (lval.sum() / float(B * N)).backward()
        kw.update(batch_kw("", cand, po, sp, y))
        kw.update(shared=np.int64(n_cand != "all"), loss_kind=str(loss), smoothing=np.float64(smoothing), input_dropout=np.float64(p_in),
                  relation_input_dropout=np.float64(p_rel), loss=np.float64(lval.item()), outputs=npy(outputs),
                  normalizer=np.float64(B * N))
        for k, p in m.named_parameters():
            kw["grad/" + k] = npy(p.grad).copy()
        m.eval()
        with torch.no_grad():
            if sp is not None:
                kw["sp_all_eval"] = npy(m.sp_prefix_score(sp[0], sp[1]))
            if po is not None:
                kw["po_all_eval"] = npy(m.po_prefix_score(po[0], po[1]))
            s, r, o = (po[1], po[0], rand_ids(rng, 2, n_ent, b_po)) if sp is None else (sp[0], sp[1], rand_ids(rng, 2, n_ent, b_sp))
            kw.update(t_subj=npy(s), t_rel=npy(r), t_obj=npy(o), triple_eval=npy(m(s, r, o)))
        save(f"g18_tucker3_{name}", **kw)


def g18_adagrad():
    seed = 1850
    rng = np.random.default_rng(seed)
    d, r_e, n_ent, n_rel, b_po, b_sp, n_cand = 12, 7, 70, 10, 7, 8, 40
    m, kw = build(seed, d, r_e, n_ent, n_rel, input_dropout=0.0, relation_input_dropout=0.0, dropout=0.0, relation_dropout=0.0)
    args = {"optimization_config": {"optimizer": "Adagrad", "epoch": 0, "lr": 0.3, "weight_decay": 1.0e-10}, "lr_scheduler_config": None}
    opts = OptimRegime.setup_optimizer_regime(args=args, model=m)
    mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0)
    mod.train()
    names = [k for k, _ in m.named_parameters()]

    def state(prefix):
        st = opts[0].optimizer.state
        for k, p in m.named_parameters():
            kw[f"{prefix}/param/{k}"] = npy(p).copy()
            kw[f"{prefix}/sum/{k}"] = npy(st[p]["sum"]).copy() if p in st else np.zeros(tuple(p.shape), np.float32)
    for step in range(3):
        cand, po, sp, y = batch(rng, n_ent, n_rel, b_po, b_sp, n_cand)
        B = b_po + b_sp
        if step == 0:                                              # (a later step starts from the state after the one before it)
            state("s0_before")
        for o in opts:
            o.update(1, step + 1)
            o.zero_grad()
        lval, _, _ = mod(inputs=[po, sp], labels=torch.from_numpy(y.copy()), use_batch_shared_entities=True, batch_shared_entities=cand,
                         epoch=1, input_style_triple_or_prefix="right_and_left_prefix")
        (lval.sum() / float(B * n_cand)).backward()
        for o in opts:
            o.step()
        state(f"s{step}_after")
        kw.update(batch_kw(f"s{step}_", cand, po, sp, y))
        kw[f"s{step}_loss"] = np.float64(lval.item())
    g = opts[0].optimizer.param_groups[0]
    kw.update({"opt_" + k: np.float64(g[k]) for k in ("lr", "eps", "weight_decay")})
    kw["n_opt_params"] = np.int64(sum(len(gr["params"]) for gr in opts[0].optimizer.param_groups))
    assert kw["n_opt_params"] == len(names)
    save("g18_tucker3_adagrad", **kw)


if __name__ == "__main__":
    g18_cases()
    g18_adagrad()
    print("torch", torch.__version__, "numpy", np.__version__)
