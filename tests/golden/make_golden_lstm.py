#!/usr/bin/env python3
"""Golden vectors for the LSTM-encoded models (g17_lstm_*), produced by running the REFERENCE itself on the CPU.

Run (never on the GPU box -- the reference is not there):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> \
        python3 -B <repo>/tests/golden/make_golden_lstm.py <reference checkout>

The script imports the unmodified reference (openkge.model / openkge.trainer / utils.optim), drives
LSTMComplexRelationModel / LSTMDistmultRelationModel with small seeded inputs (d <= 32) and stores inputs and expected
outputs as .npz fixtures next to this file.  Fixtures are DATA only.

  g17_lstm_<case>   AddLossModule forward + (loss / normalizer).backward() in training mode: the constructor's initial
                    parameters (names in order), token-id lists, batch, loss, outputs, every parameter's gradient, running
                    statistics; then eval-mode precompute_embeddings_from_tokens tables and prefix scores.  Token lists
                    include ones longer than max_len, of length 1, an empty one (all-zero token row: last wraps to
                    max_len - 1) and one with a 0 token inside.
  g17_lstm_adagrad  three steps through the reference's OptimRegime Adagrad (weight_decay 1e-10, leaked eps): the full
                    state (parameters, accumulators, running statistics) before and after every step.
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
L, VT_E, VT_R = 5, 40, 15


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


def token_map(rng, n, vocab):
    out = [[1], [1]]                                       # reserved ids 0, 1 (dataset.py:200-201)
    for i in range(2, n):
        if i == 2:
            out.append([int(rng.integers(4, vocab))])     # length 1
        elif i == 3:
            out.append([])                                 # all-zero token row: last = -1 wraps to max_len - 1
        elif i == 4:
            out.append([2, int(rng.integers(4, vocab)), 0, int(rng.integers(4, vocab)), 3])     # a 0 token inside
        else:
            k = int(rng.integers(0, L + 3))                # some longer than max_len: the tail is kept
            out.append([2] + rng.integers(4, vocab, size=k).tolist() + [3])
    return out


def flat_map(m):
    return np.array([t for row in m for t in row], np.int32), np.cumsum([0] + [len(r) for r in m]).astype(np.int64)


def build(cls, seed, d, normalize, n_ent, n_rel, rng):
    md = EntityRelationDatasetMeta(entity_id_count_map={}, relation_id_count_map={}, entity_token_id_count_map={},
                                   relation_token_id_count_map={}, entity_id_to_tokens_map=token_map(rng, n_ent, VT_E),
                                   relation_id_to_tokens_map=token_map(rng, n_rel, VT_R), entities_size=n_ent, relations_size=n_rel,
                                   min_entities_size=2, min_relations_size=2, entity_tokens_size=VT_E, relation_tokens_size=VT_R,
                                   max_length=(L, L))
    torch.manual_seed(seed)
    m = getattr(Models, cls)(entity_slot_size=d, relation_slot_size=d, train_data=md, dropout=0.0, init_std=0.3,
                             normalize=normalize, sparse=False)
    kw = dict(model=cls, seed=np.int64(seed), d=np.int64(d), normalize=str(normalize), max_len=np.int64(L),
              n_ent=np.int64(n_ent), n_rel=np.int64(n_rel), vt_e=np.int64(VT_E), vt_r=np.int64(VT_R),
              param_names=np.array([k for k, _ in m.named_parameters()]), state_keys=np.array(list(m.state_dict().keys())),
              ent_tokens=npy(m.entity_token_ids).astype(np.int32), rel_tokens=npy(m.relation_token_ids).astype(np.int32))
    kw["ent_map"], kw["ent_map_off"] = flat_map(md.entity_id_to_tokens_map)
    kw["rel_map"], kw["rel_map_off"] = flat_map(md.relation_id_to_tokens_map)
    for k, p in m.named_parameters():
        kw["init/" + k] = npy(p).copy()
    return m, kw


def batch(rng, n_ent, n_rel, b_po, b_sp, n_cand):
    cand = torch.arange(n_ent)[2:].int().unsqueeze(1) if n_cand == "all" else \
        torch.from_numpy(rng.permutation(np.arange(2, n_ent))[:n_cand].astype(np.int32)).unsqueeze(1)
    po = (rand_ids(rng, 2, n_rel, b_po), rand_ids(rng, 2, n_ent, b_po))
    sp = (rand_ids(rng, 2, n_ent, b_sp), rand_ids(rng, 2, n_rel, b_sp))
    return cand, po, sp, dense_labels(rng, b_po + b_sp, cand.shape[0])


def g17_cases():
    cases = [
        # name, class, normalize, n_ent, n_rel, d, b_po, b_sp, n_cand, loss
        ("complex_bn_all", "LSTMComplexRelationModel", "batchnorm", 60, 9, 16, 6, 7, "all", "bce"),
        ("complex_none_shared", "LSTMComplexRelationModel", None, 120, 12, 24, 8, 9, 48, "bce"),
        ("distmult_bn_shared", "LSTMDistmultRelationModel", "batchnorm", 120, 12, 32, 8, 9, 48, "bce"),
        ("distmult_none_all", "LSTMDistmultRelationModel", None, 60, 9, 16, 6, 7, "all", "bce"),
    ]
    for ci, (name, cls, normalize, n_ent, n_rel, d, b_po, b_sp, n_cand, loss) in enumerate(cases):
        rng = np.random.default_rng(1700 + ci)
        m, kw = build(cls, 1700 + ci, d, normalize, n_ent, n_rel, rng)
        m.train()
        cand, po, sp, y = batch(rng, n_ent, n_rel, b_po, b_sp, n_cand)
        B, N = y.shape
        mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), bce_label_smoothing=0.0)
        mod.train()
        lval, _, outputs = mod(inputs=[po, sp], labels=torch.from_numpy(y.copy()), use_batch_shared_entities=(n_cand != "all"),
                               batch_shared_entities=cand, epoch=1, input_style_triple_or_prefix="right_and_left_prefix")
        (lval.sum() / float(B * N)).backward()
        kw.update(cand=npy(cand), po_rel=npy(po[0]), po_obj=npy(po[1]), sp_subj=npy(sp[0]), sp_rel=npy(sp[1]), labels=y,
                  shared=np.int64(n_cand != "all"), loss=np.float64(lval.item()), outputs=npy(outputs), normalizer=np.float64(B * N))
        for k, p in m.named_parameters():
            kw["grad/" + k] = npy(p.grad).copy()
        for k, b in m.named_buffers():
            if "running" in k:
                kw["buf/" + k] = npy(b).copy()
        m.eval()
        with torch.no_grad():
            m.precompute_embeddings_from_tokens()
            kw.update(E_eval=npy(m.entity_embedding_from_tokens), R_eval=npy(m.relations_embedding_from_tokens),
                      sp_all_eval=npy(m.sp_prefix_score(sp[0], sp[1])), po_all_eval=npy(m.po_prefix_score(po[0], po[1])))
        save(f"g17_lstm_{name}", **kw)


def g17_adagrad():
    rng = np.random.default_rng(1750)
    n_ent, n_rel, d, b_po, b_sp, n_cand = 100, 10, 16, 7, 8, 40
    m, kw = build("LSTMComplexRelationModel", 1750, d, "batchnorm", n_ent, n_rel, rng)
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
            kw[f"{prefix}/sum/{k}"] = npy(st[p]["sum"]).copy() if p in st else np.zeros(tuple(p.shape), np.float32)
        for k, b in m.named_buffers():
            if "running" in k:
                kw[f"{prefix}/buf/{k}"] = npy(b).copy()
    for step in range(3):
        cand, po, sp, y = batch(rng, n_ent, n_rel, b_po, b_sp, n_cand)
        B = b_po + b_sp
        state(f"s{step}_before")
        for o in opts:
            o.update(1, step + 1)
            o.zero_grad()
        lval, _, _ = mod(inputs=[po, sp], labels=torch.from_numpy(y.copy()), use_batch_shared_entities=True, batch_shared_entities=cand,
                         epoch=1, input_style_triple_or_prefix="right_and_left_prefix")
        (lval.sum() / float(B * n_cand)).backward()
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
    save("g17_lstm_adagrad", **kw)


if __name__ == "__main__":
    g17_cases()
    g17_adagrad()
    print("torch", torch.__version__, "numpy", np.__version__)
