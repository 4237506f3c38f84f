#!/usr/bin/env python3
"""Golden vectors for the data-bias baseline models (g20_databias_*), produced by running the REFERENCE itself on the CPU.

Run (never on the GPU box -- the reference is not there):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> \
        python3 -B <repo>/tests/golden/make_golden_databias.py <reference checkout>

The script imports the unmodified reference and drives DataBiasOnlyEntityModel / DataBiasOnlyRelationModel (model.py:281-350,
:1036-1044) with the inputs, token maps and helpers of make_golden_lstm.py (d <= 32).  Fixtures are DATA only.

  g20_databias_<case>     as g17_lstm_<case>: initial parameters, token-id lists, batch, loss, outputs, every gradient the
                          backward produced, running statistics, eval tables and eval prefix scores over all entities.
                          `grad_none` lists the parameters whose .grad is None after backward() (the entity model's relation
                          slot); they have no grad/ entry.  `relation_none_po_only` has no sp direction (inputs = [po, None]).
  g20_databias_adagrad_*  three steps through the reference's OptimRegime Adagrad, as g17_lstm_adagrad: the full state before
                          and after every step.  Parameters the optimizer holds no state for (no gradient ever reached them)
                          are stored with zero `sum`s and named in `no_state`.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden_lstm import AddLossModule, OptimRegime, batch, build, npy, save  # noqa: E402  (also puts the reference on sys.path)


def call(mod, po, sp, y, cand, shared):
    return mod(inputs=[po, sp], labels=torch.from_numpy(y.copy()), use_batch_shared_entities=shared, batch_shared_entities=cand,
               epoch=1, input_style_triple_or_prefix="right_and_left_prefix")


def g20_cases():
    cases = [
        # name, class, normalize, n_ent, n_rel, d, b_po, b_sp, n_cand
        ("entity_bn_all", "DataBiasOnlyEntityModel", "batchnorm", 60, 9, 16, 6, 7, "all"),
        ("entity_none_shared", "DataBiasOnlyEntityModel", None, 120, 12, 24, 8, 9, 48),
        ("relation_bn_shared", "DataBiasOnlyRelationModel", "batchnorm", 120, 12, 32, 8, 9, 48),
        ("relation_none_po_only", "DataBiasOnlyRelationModel", None, 60, 9, 16, 6, 0, "all"),
    ]
    for ci, (name, cls, normalize, n_ent, n_rel, d, b_po, b_sp, n_cand) in enumerate(cases):
        rng = np.random.default_rng(2000 + ci)
        m, kw = build(cls, 2000 + ci, d, normalize, n_ent, n_rel, rng)
        m.train()
        cand, po, sp, y = batch(rng, n_ent, n_rel, b_po, max(b_sp, 1), n_cand)
        if b_sp == 0:                                      # no sp direction at all: the reference skips a None input
            sp, y = None, y[:b_po]
        B, N = y.shape
        mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), bce_label_smoothing=0.0)
        mod.train()
        lval, _, outputs = call(mod, po, sp, y, cand, n_cand != "all")
        (lval.sum() / float(B * N)).backward()
        kw.update(cand=npy(cand), po_rel=npy(po[0]), po_obj=npy(po[1]), labels=y, has_sp=np.int64(sp is not None),
                  shared=np.int64(n_cand != "all"), loss=np.float64(lval.item()), outputs=npy(outputs), normalizer=np.float64(B * N))
        if sp is not None:
            kw.update(sp_subj=npy(sp[0]), sp_rel=npy(sp[1]))
        none = []
        for k, p in m.named_parameters():
            if p.grad is None:
                none.append(k)
            else:
                kw["grad/" + k] = npy(p.grad).copy()
        kw["grad_none"] = np.array(none, dtype=str)
        for k, b in m.named_buffers():
            if "running" in k:
                kw["buf/" + k] = npy(b).copy()
        m.eval()
        with torch.no_grad():
            m.precompute_embeddings_from_tokens()
            kw.update(E_eval=npy(m.entity_embedding_from_tokens), R_eval=npy(m.relations_embedding_from_tokens),
                      po_all_eval=npy(m.po_prefix_score(po[0], po[1])))
            if sp is not None:
                kw["sp_all_eval"] = npy(m.sp_prefix_score(sp[0], sp[1]))
        save(f"g20_databias_{name}", **kw)


def g20_adagrad(tag, cls, seed):
    rng = np.random.default_rng(seed)
    n_ent, n_rel, d, b_po, b_sp, n_cand = 100, 10, 16, 7, 8, 40
    m, kw = build(cls, seed, d, "batchnorm", n_ent, n_rel, rng)
    m.train()
    args = {"optimization_config": {"optimizer": "Adagrad", "epoch": 0, "lr": 0.1, "weight_decay": 1.0e-10}, "lr_scheduler_config": None}
    opts = OptimRegime.setup_optimizer_regime(args=args, model=m)
    mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0)
    mod.train()
    names = [k for k, _ in m.named_parameters()]

    def state(prefix):
        st = opts[0].optimizer.state
        for k, p in m.named_parameters():
            kw[f"{prefix}/param/{k}"] = npy(p).copy()
            kw[f"{prefix}/sum/{k}"] = npy(st[p]["sum"]).copy() if p in st and "sum" in st[p] else np.zeros(tuple(p.shape), np.float32)
        for k, b in m.named_buffers():
            if "running" in k:
                kw[f"{prefix}/buf/{k}"] = npy(b).copy()
    grad_none = None
    for step in range(3):
        cand, po, sp, y = batch(rng, n_ent, n_rel, b_po, b_sp, n_cand)
        B = b_po + b_sp
        state(f"s{step}_before")
        for o in opts:
            o.update(1, step + 1)
            o.zero_grad()
        lval, _, _ = call(mod, po, sp, y, cand, True)
        (lval.sum() / float(B * n_cand)).backward()
        none = [k for k, p in m.named_parameters() if p.grad is None]
        assert grad_none is None or grad_none == none
        grad_none = none
        for o in opts:
            o.step()
        state(f"s{step}_after")
        kw.update({f"s{step}_cand": npy(cand), f"s{step}_po_rel": npy(po[0]), f"s{step}_po_obj": npy(po[1]),
                   f"s{step}_sp_subj": npy(sp[0]), f"s{step}_sp_rel": npy(sp[1]), f"s{step}_labels": y,
                   f"s{step}_loss": np.float64(lval.item())})
    g = opts[0].optimizer.param_groups[0]
    kw.update({"opt_" + k: np.float64(g[k]) for k in ("lr", "eps", "weight_decay")})
    kw["n_opt_params"] = np.int64(sum(len(gr["params"]) for gr in opts[0].optimizer.param_groups))
    assert kw["n_opt_params"] == len(names)
    st = opts[0].optimizer.state
    # (torch's Adagrad creates its `sum` state for every parameter at construction: "no state" is told by what a step leaves
    #  behind -- a parameter no gradient reached keeps step == 0 and an all-zero sum)
    kw["no_state"] = np.array([k for k, p in m.named_parameters()
                               if p not in st or "sum" not in st[p] or float(st[p].get("step", 0)) == 0], dtype=str)
    kw["grad_none"] = np.array(grad_none, dtype=str)
    save(f"g20_databias_adagrad_{tag}", **kw)


if __name__ == "__main__":
    g20_cases()
    g20_adagrad("entity", "DataBiasOnlyEntityModel", 2050)
    g20_adagrad("relation", "DataBiasOnlyRelationModel", 2051)
    print("torch", torch.__version__, "numpy", np.__version__)
