"""Golden vectors of the reference's SPARSE training step (CPU, where the reference is mounted only).

  g21_sparse_{complex,distmult}   Lookup*RelationModel(sparse=True) -> nn.Embedding(sparse=True) (model.py:390-391),
                                  AddLossModule (BCE, reduction='sum') and torch.optim.Adagrad(lr=0.3, weight_decay=0,
                                  eps=1e-8): three steps on batch-shared candidates (N = 24 ids, |E| = 66, |R| = 10, d = 16,
                                  b = 8), dropout 0.  Entities repeat among the prefixes and between prefixes and candidates;
                                  step 1 has only sp rows.  Stored: inputs, tables and `sum` after every step.

The same three steps are also run with sparse=False (dense gradients, dense Adagrad at weight_decay = 0) from the same
initial tables: the reference's own sparse-against-dense difference is printed and stored (`ref_sparse_vs_dense`), and the
generator refuses a seed for which it is not at least 10x inside the G3 bound of tests/test_oracle_golden.py
(torch's coalesce() sums in an order of its own, so tests against this golden are tolerances, not bit-equality).

    python tests/golden/make_golden_sparse.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
assert os.path.isdir("/root/reference"), "golden vectors can only be generated where the reference is mounted"
if "/root/reference" not in sys.path:
    sys.path.insert(0, "/root/reference")

from openkge.dataset import EntityRelationDatasetMeta  # noqa: E402
from openkge.model import Models  # noqa: E402
from openkge.trainer import AddLossModule  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(4)
N_ENT, N_REL, D, B, N_CAND, LR, EPS, SEED = 66, 10, 16, 8, 24, 0.3, 1e-8, 53


def meta(n_ent, n_rel):
    return EntityRelationDatasetMeta(
        entity_id_count_map={}, relation_id_count_map={}, entity_token_id_count_map={},
        relation_token_id_count_map={}, entity_id_to_tokens_map={}, relation_id_to_tokens_map={},
        entities_size=n_ent, relations_size=n_rel, min_entities_size=2, min_relations_size=2,
        entity_tokens_size=4, relation_tokens_size=4, max_length=1,
    )


def npy(t):
    return t.detach().cpu().numpy()


def col(a):
    return torch.from_numpy(np.asarray(a, np.int32).reshape(-1, 1))


def make_batches(rng):
    """three batches; prefix entities are drawn from a pool of six ids of which three are also candidates"""
    batches = []
    for step in range(3):
        cand = rng.permutation(np.arange(2, N_ENT))[:N_CAND].astype(np.int32)
        pool = np.concatenate([cand[:3], rng.permutation(np.setdiff1d(np.arange(2, N_ENT), cand))[:3]])
        n_po = 0 if step == 1 else B // 2
        n_sp = B - n_po
        po = (rng.integers(2, N_REL, n_po).astype(np.int32), rng.choice(pool, n_po).astype(np.int32)) if n_po else None
        sp = (rng.choice(pool, n_sp).astype(np.int32), rng.integers(2, N_REL, n_sp).astype(np.int32))
        y = np.zeros((B, N_CAND), np.float32)
        for r in range(B):
            y[r, rng.choice(N_CAND, size=rng.integers(1, 4), replace=False)] = 1
        batches.append(dict(cand=cand, po=po, sp=sp, labels=y))
    return batches


def run(mname, sparse, batches, init):
    torch.manual_seed(SEED)
    m = getattr(Models, mname)(entity_slot_size=D, input_dropout=0.0, init_std=0.1, sparse=sparse, train_data=meta(N_ENT, N_REL))
    if init is not None:
        with torch.no_grad():
            m.entity_embedding.weight.copy_(torch.from_numpy(init[0]))
            m.relation_embedding.weight.copy_(torch.from_numpy(init[1]))
    m.train()
    E0, R0 = npy(m.entity_embedding.weight).copy(), npy(m.relation_embedding.weight).copy()
    opt = torch.optim.Adagrad(m.parameters(), lr=LR, weight_decay=0, eps=EPS)
    mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0)
    mod.train()
    steps = []
    for b in batches:
        po = None if b["po"] is None else (col(b["po"][0]), col(b["po"][1]))
        sp = (col(b["sp"][0]), col(b["sp"][1]))
        opt.zero_grad()
        loss, _, _ = mod(inputs=[po, sp], labels=torch.from_numpy(b["labels"].copy()), use_batch_shared_entities=True,
                         batch_shared_entities=col(b["cand"]), epoch=1, input_style_triple_or_prefix="right_and_left_prefix")
        (loss.sum() / float(B * N_CAND)).backward()
        assert m.entity_embedding.weight.grad.is_sparse == sparse
        opt.step()
        steps.append(dict(loss=np.float64(loss.item()), E=npy(m.entity_embedding.weight).copy(), R=npy(m.relation_embedding.weight).copy(),
                          sumE=npy(opt.state[m.entity_embedding.weight]["sum"]).copy(),
                          sumR=npy(opt.state[m.relation_embedding.weight]["sum"]).copy()))
    return E0, R0, steps


def adagrad_tol(sum_ref, sum_prev, lr, eps, rel_dg=1e-6):
    """the G3 bound of tests/test_oracle_golden.py"""
    dg = rel_dg * np.sqrt(np.maximum(sum_ref - sum_prev, 0).max())
    return 2e-6 + lr * dg / (np.sqrt(sum_ref) + eps)


def main():
    for mname, tag in (("LookupComplexRelationModel", "complex"), ("LookupDistmultRelationModel", "distmult")):
        batches = make_batches(np.random.default_rng(SEED))
        E0, R0, sp_steps = run(mname, True, batches, None)
        _, _, de_steps = run(mname, False, batches, (E0, R0))
        worst, worst_abs = 0.0, 0.0
        for i, (a, b) in enumerate(zip(sp_steps, de_steps)):
            for k, ks, p0 in (("E", "sumE", E0), ("R", "sumR", R0)):
                prev = np.zeros_like(p0) if i == 0 else sp_steps[i - 1][ks]
                tol = adagrad_tol(a[ks], prev, LR, EPS)
                worst = max(worst, float((np.abs(a[k] - b[k]) / tol).max()))
                worst_abs = max(worst_abs, float(np.abs(a[k] - b[k]).max()))
        print(tag, "reference sparse vs dense: max |diff| =", worst_abs, " max diff / G3 bound =", worst)
        assert worst <= 0.1, "pick another seed: the reference's own sparse-vs-dense difference must stay 10x inside the G3 bound"
        kw = dict(E0=E0, R0=R0, nsteps=np.int64(3), opt_lr=np.float64(LR), opt_eps=np.float64(EPS), opt_weight_decay=np.float64(0.0),
                  ref_sparse_vs_dense=np.float64(worst_abs), ref_sparse_vs_dense_over_bound=np.float64(worst))
        for i, (b, s) in enumerate(zip(batches, sp_steps)):
            kw[f"s{i}_cand"] = b["cand"]
            kw[f"s{i}_labels"] = b["labels"]
            kw[f"s{i}_po_rel"] = b["po"][0] if b["po"] is not None else np.zeros(0, np.int32)
            kw[f"s{i}_po_obj"] = b["po"][1] if b["po"] is not None else np.zeros(0, np.int32)
            kw[f"s{i}_sp_subj"], kw[f"s{i}_sp_rel"] = b["sp"]
            for k, v in s.items():
                kw[f"s{i}_{k}"] = v
        path = os.path.join(OUT, f"g21_sparse_{tag}.npz")
        np.savez_compressed(path, **kw)
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
