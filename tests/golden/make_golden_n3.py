"""Golden vectors of the reference's `l2_reg` hook (openkge/model.py:444-453, :471-479) -- G23.

Run where the unmodified reference is mounted, on the CPU, as make_golden.py is:

    python tests/golden/make_golden_n3.py

  g23_n3_*   LookupComplexRelationModel / LookupDistmultRelationModel with l2_reg > 0 as the ONLY _encode variant, in training
             mode through the reference's AddLossModule and the Trainer's backward_loss = (loss + hook) / normalizer
             (trainer.py:217-222): loss, hook, outputs, the gradient of both tables, and -- with dropout on -- the Bernoulli
             keep masks the reference drew, captured from the same generator state as G2 does (one F.dropout per mask, in the
             order of the reference's _encode calls), input_dropout and dropout of one call folded into one keep mask.
    complex_noshare_both   batch_shared_entities None, po and sp rows: the candidate block is encoded once per direction
    complex_noshare_po     batch_shared_entities None, po rows only: once
    distmult_repeat        a sampled shared id list that names some entities twice and one three times
    complex_dropout        input_dropout 0.3, dropout 0.2: the hook divides the rows by 0.2 (the probability), relation rows too
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden import AddLossModule, Models, dense_labels, meta, npy, rand_ids, save  # noqa: E402

F = torch.nn.functional


def keep_mask(rows, d, p_in, p_out):
    """the keep mask of one _encode call: F.dropout(p_in) then F.dropout(p_out) on (rows, d), as model.py:461-470 draws them"""
    keep = torch.ones(rows, d, dtype=torch.bool)
    for p in (p_in, p_out):
        if p > 0:
            keep &= F.dropout(torch.ones(rows, d), p=p, training=True) > 0
    return keep


def run(name, mname, n_ent, n_rel, d, b_po, b_sp, cand_mode, seed, l2_reg, input_dropout=0.0, dropout=0.0):
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    m = getattr(Models, mname)(entity_slot_size=d, input_dropout=input_dropout, dropout=dropout, init_std=0.3, sparse=False,
                               train_data=meta(n_ent, n_rel), l2_reg=l2_reg)
    m.train()
    E0, R0 = npy(m.entity_embedding.weight).copy(), npy(m.relation_embedding.weight).copy()
    no_shared = cand_mode == "noshare"
    if cand_mode in ("noshare", "all"):
        cand = torch.arange(n_ent)[2:].int().unsqueeze(1)
    else:                                                    # a sampled list WITH repeats
        ids = rng.integers(2, n_ent, size=int(cand_mode)).astype(np.int32)
        ids[3], ids[7], ids[11] = ids[0], ids[0], ids[5]     # one id three times, one twice (on top of what the draw repeats)
        cand = torch.from_numpy(ids).unsqueeze(1)
    N = cand.shape[0]
    po = (rand_ids(rng, 2, n_rel, b_po), rand_ids(rng, 2, n_ent, b_po)) if b_po else None
    sp = (rand_ids(rng, 2, n_ent, b_sp), rand_ids(rng, 2, n_rel, b_sp)) if b_sp else None
    B = b_po + b_sp
    y = dense_labels(rng, B, N)
    mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0)
    mod.train()
    masks = {}
    if input_dropout > 0 or dropout > 0:
        # the reference's draw order with a shared list: candidates (precompute_batch_shared_inputs), the po objects, the sp
        # subjects; the relation rows draw nothing (relation_dropout = relation_input_dropout = 0)
        assert not no_shared
        st = torch.get_rng_state()
        torch.manual_seed(seed + 77)
        masks["mask_cand"] = keep_mask(N, d, input_dropout, dropout)
        if b_po:
            masks["mask_po_ent"] = keep_mask(b_po, d, input_dropout, dropout)
        if b_sp:
            masks["mask_sp_ent"] = keep_mask(b_sp, d, input_dropout, dropout)
        torch.set_rng_state(st)
        torch.manual_seed(seed + 77)
    loss, hook, outputs = mod(inputs=[po, sp], labels=torch.from_numpy(y.copy()), use_batch_shared_entities=cand_mode.isdigit(),
                              batch_shared_entities=None if no_shared else cand, epoch=1,
                              input_style_triple_or_prefix="right_and_left_prefix")
    assert hook is not None
    normalizer = float(B * N)
    ((loss.sum() + hook) / normalizer).backward()
    out = dict(model=np.str_("complex" if "Complex" in mname else "distmult"), E=E0, R=R0, cand=npy(cand), labels=y,
               loss=np.float64(loss.item()), hook=np.float64(hook.item()), outputs=npy(outputs),
               dE=npy(m.entity_embedding.weight.grad), dR=npy(m.relation_embedding.weight.grad),
               normalizer=np.float64(normalizer), l2_reg=np.float64(l2_reg), input_dropout=np.float64(input_dropout),
               dropout=np.float64(dropout), no_shared=np.bool_(no_shared), shared_list=np.bool_(cand_mode.isdigit()))
    if po is not None:
        out.update(po_rel=npy(po[0]), po_obj=npy(po[1]))
    if sp is not None:
        out.update(sp_subj=npy(sp[0]), sp_rel=npy(sp[1]))
    for k, v in masks.items():
        out[k] = npy(v).astype(np.uint8)
    save("g23_n3_" + name, **out)


def g23():
    C, D = "LookupComplexRelationModel", "LookupDistmultRelationModel"
    run("complex_noshare_both", C, 60, 8, 16, 6, 5, "noshare", 231, 0.01)
    run("complex_noshare_po", C, 60, 8, 16, 7, 0, "noshare", 232, 0.01)
    run("distmult_repeat", D, 90, 9, 13, 5, 6, "40", 233, 0.02)
    run("complex_dropout", C, 60, 8, 16, 6, 5, "all", 234, 0.01, input_dropout=0.3, dropout=0.2)


if __name__ == "__main__":
    g23()
