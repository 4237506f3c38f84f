"""Golden vectors of the reference at slot sizes above 512 (CPU, where the reference is mounted only).

  g22_wide_complex_d516    LookupComplexRelationModel,  entity_slot_size 516 (halves of 258)
  g22_wide_distmult_d513   LookupDistmultRelationModel, entity_slot_size 513 (odd)

|E| = 40, |R| = 6, 6 po + 5 sp rows, 1-vs-all (N = 38), dropout 0.  The SAME tables, ids and labels go through AddLossModule
twice: BCEWithLogitsLoss(sum) with label smoothing 0.1 (keys bce_*) and KLDivLoss(sum) (keys kl_*), each followed by
(loss / (B N)).backward().  Stored: E, R, the ids, labels, and per loss: loss, all_outputs, dE, dR.  Data only.

    python tests/golden/make_golden_wide.py
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
N_ENT, N_REL, B_PO, B_SP, SMOOTHING = 40, 6, 6, 5, 0.1


def meta(n_ent, n_rel):
    return EntityRelationDatasetMeta(
        entity_id_count_map={}, relation_id_count_map={}, entity_token_id_count_map={},
        relation_token_id_count_map={}, entity_id_to_tokens_map={}, relation_id_to_tokens_map={},
        entities_size=n_ent, relations_size=n_rel, min_entities_size=2, min_relations_size=2,
        entity_tokens_size=4, relation_tokens_size=4, max_length=1,
    )


def npy(t):
    return t.detach().cpu().numpy()


def ids(rng, lo, hi, n):
    return torch.from_numpy(rng.integers(lo, hi, size=(n, 1)).astype(np.int32))


def main():
    for mname, tag, d, seed in (("LookupComplexRelationModel", "complex", 516, 221), ("LookupDistmultRelationModel", "distmult", 513, 222)):
        rng = np.random.default_rng(seed)
        po = (ids(rng, 2, N_REL, B_PO), ids(rng, 2, N_ENT, B_PO))
        sp = (ids(rng, 2, N_ENT, B_SP), ids(rng, 2, N_REL, B_SP))
        cand = torch.arange(N_ENT)[2:].int().unsqueeze(1)
        B, N = B_PO + B_SP, cand.shape[0]
        y = np.zeros((B, N), np.float32)
        for b in range(B):
            y[b, rng.choice(N, size=int(rng.integers(1, 5)), replace=False)] = 1.0
        kw = dict(cand=npy(cand), labels=y, po_rel=npy(po[0]), po_obj=npy(po[1]), sp_subj=npy(sp[0]), sp_rel=npy(sp[1]),
                  normalizer=np.float64(B * N), smoothing=np.float64(SMOOTHING))
        for loss_kind in ("bce", "kl"):
            torch.manual_seed(seed)                  # the same tables for both losses
            m = getattr(Models, mname)(entity_slot_size=d, input_dropout=0.0, init_std=0.1, sparse=False, train_data=meta(N_ENT, N_REL))
            m.train()
            loss_fn = torch.nn.BCEWithLogitsLoss(reduction="sum") if loss_kind == "bce" else torch.nn.KLDivLoss(reduction="sum")
            mod = AddLossModule(m, loss_fn, bce_label_smoothing=SMOOTHING if loss_kind == "bce" else 0.0)
            mod.train()
            out_loss, hook, outputs = mod(inputs=[po, sp], labels=torch.from_numpy(y.copy()), use_batch_shared_entities=False,
                                          batch_shared_entities=cand, epoch=1, input_style_triple_or_prefix="right_and_left_prefix")
            assert hook is None
            (out_loss.sum() / float(B * N)).backward()
            E, R = npy(m.entity_embedding.weight), npy(m.relation_embedding.weight)
            if "E" in kw:
                assert np.array_equal(kw["E"], E) and np.array_equal(kw["R"], R)
            kw.update(E=E, R=R)
            kw.update({f"{loss_kind}_loss": np.float64(out_loss.item()), f"{loss_kind}_outputs": npy(outputs),
                       f"{loss_kind}_dE": npy(m.entity_embedding.weight.grad), f"{loss_kind}_dR": npy(m.relation_embedding.weight.grad)})
        path = os.path.join(OUT, f"g22_wide_{tag}_d{d}.npz")
        np.savez_compressed(path, **kw)
        print("wrote", path, os.path.getsize(path), "bytes")
    print("torch", torch.__version__, "numpy", np.__version__)


if __name__ == "__main__":
    main()
