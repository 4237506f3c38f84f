#!/usr/bin/env python3
"""Golden vectors for the checkpoints of the token-encoded and Tucker3 models (g22_ckpt_*), produced by running the REFERENCE
itself on the CPU.

Run (never on the GPU box -- the reference is not there):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> \
        python3 -B <repo>/tests/golden/make_golden_ckpt.py <reference checkout>

The script imports the unmodified reference through the builders of make_golden_lstm.py / make_golden_bigram.py (with its id ->
token shim) / make_golden_tucker3.py, trains each model for three steps of AddLossModule + OptimRegime and stores, as DATA only,

  <init>      the seeded initial state_dict ("sd0/<key>"), next to what the builder stores (token maps, sizes, seed, init/)
  <batches>   three fixed batches "s{0,1,2}_*" (batch-shared candidates, dropout 0) and their losses
  <run>ckpt   the dict Trainer.save (trainer.py:608-622) holds after TWO steps, without its pickled `results`: every tensor under
              "<run>ckpt/<path>", path = "state_dict/<key>" or "optimizer/<param index>/<state key>"; "<run>ckpt_keys" lists the
              paths in the checkpoint's own order, "<run>ckpt_shapes" / "<run>ckpt_dtypes" their shapes ("7x16", "" = 0-d) and
              torch dtypes; "<run>ckpt_meta" is the rest as JSON (epoch, training_steps, param_groups, regime)
  <run>end    the same paths after step THREE ("<run>end/<path>")

<run> is "" for `optimizer: Adagrad` (lr 0.3, weight_decay 1e-10, the regime's leaked eps) and "adam_" for the second run the
unigram and LSTM fixtures carry (`optimizer: Adam`, lr 0.01, weight_decay 1e-10).  The *_adagrad fixtures of g16-g20 hold
parameters and `sum`s of similar runs, but neither the checkpoint's key order, dtypes, `step` entries, param_groups and
num_batches_tracked nor this learning rate: nothing of them is repeated here.
"""
import copy
import json
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden_bigram as BG  # noqa: E402  (each puts the reference on sys.path)
import make_golden_lstm as LS  # noqa: E402
import make_golden_tucker3 as T3  # noqa: E402
from make_golden_lstm import AddLossModule, OptimRegime, npy, save  # noqa: E402

REGIMES = {"": {"optimizer": "Adagrad", "epoch": 0, "lr": 0.3, "weight_decay": 1.0e-10},
           "adam_": {"optimizer": "Adam", "epoch": 0, "lr": 0.01, "weight_decay": 1.0e-10}}


def flatten(ckpt):
    """-> ([(path, tensor)] in the checkpoint's order, everything else as a JSON string)"""
    out = [("state_dict/" + k, v) for k, v in ckpt["state_dict"].items()]
    assert len(ckpt["optimizer_state_dict"]) == 1
    reg = ckpt["optimizer_state_dict"][0]
    for i, st in reg["optimizer_state"]["state"].items():
        out += [(f"optimizer/{i}/{k}", v) for k, v in st.items()]
    meta = {"epoch": ckpt["epoch"], "training_steps": ckpt["training_steps"], "param_groups": reg["optimizer_state"]["param_groups"],
            "regime": reg["regime"], "top_level_keys": list(ckpt.keys())}
    return out, json.dumps(meta)


def store(kw, prefix, ckpt, with_keys):
    flat, meta = flatten(ckpt)
    for path, t in flat:
        kw[f"{prefix}/{path}"] = npy(t).copy()
    if with_keys:
        kw[prefix + "_keys"] = np.array([p for p, _ in flat])
        kw[prefix + "_shapes"] = np.array(["x".join(str(n) for n in t.shape) for _, t in flat])
        kw[prefix + "_dtypes"] = np.array([str(t.dtype) for _, t in flat])
        kw[prefix + "_meta"] = meta


def run(kw, run_prefix, make, batches):
    """three steps of AddLossModule + OptimRegime on a freshly built model; the Trainer.save dict after steps two and three"""
    m = make()
    m.train()
    args = {"optimization_config": dict(REGIMES[run_prefix]), "lr_scheduler_config": None}
    opts = OptimRegime.setup_optimizer_regime(args=args, model=m)
    mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0)
    mod.train()
    for step, (cand, po, sp, y) in enumerate(batches):
        B, N = y.shape
        for o in opts:
            o.update(1, step + 1)
            o.zero_grad()
        lval, _, _ = mod(inputs=[po, sp], labels=torch.from_numpy(y.copy()), use_batch_shared_entities=True, batch_shared_entities=cand,
                         epoch=1, input_style_triple_or_prefix="right_and_left_prefix")
        (lval.sum() / float(B * N)).backward()
        for o in opts:
            o.step()
        kw[f"{run_prefix}s{step}_loss"] = np.float64(lval.item())
        if step >= 1:
            state = {"epoch": 1, "training_steps": step + 1, "state_dict": m.state_dict(),
                     "optimizer_state_dict": [o.state_dict() for o in opts], "validation_results": None}
            store(kw, run_prefix + ("ckpt" if step == 1 else "end"), copy.deepcopy(state), with_keys=step == 1)


def fixture(name, build, batch, runs=("",)):
    """build() -> (model, builder kw), the same parameters at every call; batch(rng) -> (cand, po, sp, labels)"""
    m, kw = build()
    for k, v in m.state_dict().items():
        kw["sd0/" + k] = npy(v).copy()
    rng = np.random.default_rng(int(kw["seed"]) + 1)
    batches = [batch(rng) for _ in range(3)]
    for s, (cand, po, sp, y) in enumerate(batches):
        kw.update({f"s{s}_cand": npy(cand), f"s{s}_po_rel": npy(po[0]), f"s{s}_po_obj": npy(po[1]), f"s{s}_sp_subj": npy(sp[0]),
                   f"s{s}_sp_rel": npy(sp[1]), f"s{s}_labels": y})
    for r in runs:
        run(kw, r, lambda: build()[0], batches)
    kw["runs"] = np.array(list(runs))
    save("g22_ckpt_" + name, **kw)


def lstm_like(cls, seed, d, n_ent, n_rel, shim=False):
    def build():
        m, kw = LS.build(cls, seed, d, "batchnorm", n_ent, n_rel, np.random.default_rng(seed))
        if shim:
            m.entity_projection = None          # (the attribute model.py:789 reads and the unigram constructor never sets)
            kw["pool"] = "sum"
        return m, kw
    return build, lambda rng: LS.batch(rng, n_ent, n_rel, 7, 8, 40)


def bigram():
    seed, d, n_ent, n_rel = 2203, 8, 100, 10
    return (lambda: BG.build("BigramPoolingComplexRelationModel", seed, d, "batchnorm", "sum", n_ent, n_rel, np.random.default_rng(seed)),
            lambda rng: BG.batch(rng, n_ent, n_rel, 7, 8, 40))


def tucker3():
    seed, d, r_e, n_ent, n_rel = 2204, 12, 7, 70, 10
    return (lambda: T3.build(seed, d, r_e, n_ent, n_rel, input_dropout=0.0, relation_input_dropout=0.0, dropout=0.0, relation_dropout=0.0),
            lambda rng: T3.batch(rng, n_ent, n_rel, 7, 8, 40))


if __name__ == "__main__":
    fixture("unigram", *lstm_like("UnigramPoolingComplexRelationModel", 2200, 16, 70, 9, shim=True), runs=("", "adam_"))
    fixture("lstm", *lstm_like("LSTMComplexRelationModel", 2201, 16, 100, 10), runs=("", "adam_"))
    fixture("bias_entity", *lstm_like("DataBiasOnlyEntityModel", 2202, 16, 100, 10))
    fixture("bigram", *bigram())
    fixture("tucker3", *tucker3())
    print("torch", torch.__version__, "numpy", np.__version__)
