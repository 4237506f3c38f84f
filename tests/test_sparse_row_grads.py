"""okge_train_forward_backward(OKGE_TRAIN_ROW_GRADS): gradients in occurrence rows, against the existing dense path on the
RELABELLED problem -- tables whose rows are the occurrences (EV = E[occurrence ids], RV likewise, built here with torch
indexing), positions for ids, OKGE_TRAIN_DISTINCT_PREFIX_ROWS -- every gradient row and the loss, BIT FOR BIT.

Route taken (include/okge.h): the library gathers the occurrence rows into two small tables behind the
step's scratch and runs the tile kernels every other caller runs, untouched -- so what this file pins is the gather, the position
ids, the flag handling and the dropout keying, through every launch shape of the step.

Dropout: the Philox counter is keyed by POSITION (candidate column / batch row, include/okge.h okge_dropout), not by entity id,
so the relabelled problem draws the masks of the original one and the comparison is bit for bit at input dropout 0.4 too.

Write sites of table gradients and the case that reaches each (B = n_po + n_sp):
  store_tile_gradient (okge_tile.h), fused_tile64_kernel     every d <= 256 case, B <= 64 (one row block: direct stores)
  fused_tile64k_kernel, whole-segment stores                 d = 264, 512 (stream-K launch, the default above 256)
  dc_reduce_streamk_kernel                                   d = 264, 512 with N = 70, 130 (tiles shared between workgroups)
  fused_tile64k_kernel as a (tile, row split) grid           test_launch_shapes[streamk_off]: OKGE_STREAMK=0, d = 512
  dc_reduce_kernel (batch split)                             test_launch_shapes[b_split]: OKGE_B_SPLIT=2, B = 77 (two row blocks),
                                                             d = 200 and d = 512 (with OKGE_STREAMK=0)
  dc_reduce_kernel (tail split)                              NOT reachable at test size: it needs more candidate tiles than
                                                             compute units (N > 16384); it is the kernel of the batch split, and
                                                             test_launch_shapes[tail_split_off] pins OKGE_TAIL_SPLIT=0 all the same
  prefix_backward_vec_kernel<1>                              ComplEx d % 8 == 0 / DistMult d % 4 == 0, N <= 130 (fewer than 8 tiles)
  prefix_backward_vec_kernel<8>                              test_launch_shapes[dq_split8]: N = 600 (eight and more dQ slabs)
  prefix_backward_kernel                                     ComplEx d = 6, DistMult d = 5 (no 16-byte columns)
"""
import numpy as np
import pytest
import torch

from open_knowledge_graph_embeddings_amd import hotpath as H

N_ENT, N_REL = 300, 11
SPLITS = [(3, 5), (0, 7), (6, 0)]
NS = [1, 63, 70, 130]


def _problem(seed, d, n, n_po, n_sp):
    g = torch.Generator().manual_seed(seed)
    E = (torch.randn(N_ENT, d, generator=g) * 0.3).cuda()
    R = (torch.randn(N_REL, d, generator=g) * 0.3).cuda()
    cand = torch.randperm(N_ENT - 2, generator=g)[:n].to(torch.int32) + 2
    if n > N_ENT - 2:                                               # (more candidates than entities: ids repeat freely)
        cand = torch.randint(2, N_ENT, (n,), generator=g, dtype=torch.int32)
    if n > 1:
        cand[n - 1] = cand[0]                                       # a repeated candidate id
    B = n_po + n_sp
    ent = torch.randint(2, N_ENT, (B,), generator=g, dtype=torch.int32)
    ent[0] = cand[0]                                                # a prefix entity that is also a candidate
    if B > 2:
        ent[2] = ent[1]                                             # and one that repeats among the prefixes
    rel = torch.randint(2, N_REL, (B,), generator=g, dtype=torch.int32)
    rows, cols = [], []
    for r in range(B):
        for c in torch.randperm(n, generator=g)[:min(n, 3)].tolist():
            rows.append(r)
            cols.append(c)
    order = np.argsort(np.asarray(cols), kind="stable")
    prow = torch.tensor(np.asarray(rows)[order], dtype=torch.int32).cuda()
    pcol = torch.tensor(np.asarray(cols)[order], dtype=torch.int32).cuda()
    return E, R, cand.cuda(), ent.cuda(), rel.cuda(), prow, pcol


def _batches(cand, ent, rel, prow, pcol, n, n_po, n_sp, p_drop):
    """the original batch and its relabelled twin (positions for ids), with one set of dropout specs"""
    drops = H.dropout_specs(p_drop, p_drop / 2, seed=7, step=3)
    kw = dict(drop_cand=drops[0], drop_po_ent=drops[1], drop_po_rel=drops[2], drop_sp_ent=drops[3], drop_sp_rel=drops[4],
              pos_row=prow, pos_col=pcol)
    part = lambda x, lo, hi: x[lo:hi].contiguous() if hi > lo else None          # noqa: E731
    B = n_po + n_sp
    real = H.PrefixBatch(po_rel=part(rel, 0, n_po), po_obj=part(ent, 0, n_po), sp_subj=part(ent, n_po, B), sp_rel=part(rel, n_po, B),
                         cand_ids=cand, **kw)
    pe = torch.arange(n, n + B, dtype=torch.int32, device="cuda")
    pr = torch.arange(B, dtype=torch.int32, device="cuda")
    twin = H.PrefixBatch(po_rel=part(pr, 0, n_po), po_obj=part(pe, 0, n_po), sp_subj=part(pe, n_po, B), sp_rel=part(pr, n_po, B),
                         cand_first=0, n_cand=n, **kw)
    ids_e = torch.cat([cand, ent]).long()
    return real, twin, ids_e, rel.long()


def _compare(hp, scorer, d, n, n_po, n_sp, loss, p_drop, seed):
    E, R, cand, ent, rel, prow, pcol = _problem(seed, d, n, n_po, n_sp)
    real, twin, ids_e, ids_r = _batches(cand, ent, rel, prow, pcol, n, n_po, n_sp, p_drop)
    B = n_po + n_sp
    smoothing = 0.1 if loss == "bce" else 0.0
    EV, RV = E[ids_e].contiguous(), R[ids_r].contiguous()
    dEV, dRV = torch.full_like(EV, float("nan")), torch.full_like(RV, float("nan"))
    ref_loss = hp.forward_backward(EV, RV, scorer, twin, dEV, dRV, loss=loss, label_smoothing=smoothing, grads_zero=True,
                                   distinct_prefix_rows=True).clone()
    gE = torch.full((n + B, d), float("nan"), device="cuda")          # may hold anything on entry: every row is stored
    gR = torch.full((B, d), float("nan"), device="cuda")
    got_loss = hp.forward_backward(E, R, scorer, real, gE, gR, loss=loss, label_smoothing=smoothing, row_grads=True)
    tag = (scorer, d, n, n_po, n_sp, loss, p_drop)
    assert torch.equal(got_loss.view(torch.int64), ref_loss.view(torch.int64)), tag
    assert not torch.isnan(dEV).any() and not torch.isnan(dRV).any(), tag
    assert torch.equal(gE.view(torch.int32), dEV.view(torch.int32)), tag
    assert torch.equal(gR.view(torch.int32), dRV.view(torch.int32)), tag
    if n > 1 or loss == "bce":                                        # (KL over ONE candidate: softmax = 1, the gradient is exactly zero)
        assert float(gE.abs().max()) > 0 and float(gR.abs().max()) > 0, tag


@pytest.mark.gpu
@pytest.mark.parametrize("scorer,d", [("complex", d) for d in (6, 8, 64, 72, 200, 208, 256, 264, 512)] + [("distmult", 5), ("distmult", 512)])
def test_row_grads_equal_relabelled_dense_path(okge_lib, scorer, d):
    hp = H.HotPath("cuda:0")
    seed = 0
    for n in NS:
        for n_po, n_sp in SPLITS:
            for loss in ("bce", "kl"):
                for p_drop in (0.0, 0.4):
                    seed += 1
                    _compare(hp, scorer, d, n, n_po, n_sp, loss, p_drop, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["b_split", "streamk_off", "tail_split_off", "dq_split8"])
def test_launch_shapes(okge_lib, monkeypatch, case):
    """the launch shapes a small problem does not take by itself (see the table in the module docstring)"""
    hp = H.HotPath("cuda:0")
    if case == "b_split":
        monkeypatch.setenv("OKGE_B_SPLIT", "2")
        for d, streamk in ((200, "1"), (512, "0")):
            monkeypatch.setenv("OKGE_STREAMK", streamk)
            for loss in ("bce", "kl"):
                _compare(hp, "complex", d, 130, 40, 37, loss, 0.4, 100 + d)
    elif case == "streamk_off":
        monkeypatch.setenv("OKGE_STREAMK", "0")
        for n in (70, 130):
            _compare(hp, "complex", 512, n, 3, 5, "bce", 0.4, 200 + n)
            _compare(hp, "distmult", 512, n, 0, 7, "kl", 0.0, 300 + n)
    elif case == "dq_split8":
        _compare(hp, "complex", 64, 600, 3, 5, "bce", 0.4, 500)
        _compare(hp, "distmult", 512, 600, 3, 5, "kl", 0.4, 501)
    else:
        monkeypatch.setenv("OKGE_TAIL_SPLIT", "0")
        _compare(hp, "complex", 200, 130, 3, 5, "bce", 0.4, 400)


@pytest.mark.gpu
def test_row_grads_refusals_and_contiguous_range(okge_lib):
    from open_knowledge_graph_embeddings_amd import _native as N
    hp = H.HotPath("cuda:0")
    d, n, n_po, n_sp = 64, 70, 3, 5
    E, R, cand, ent, rel, prow, pcol = _problem(9, d, n, n_po, n_sp)
    real, _, _, _ = _batches(cand, ent, rel, prow, pcol, n, n_po, n_sp, 0.0)
    with pytest.raises(N.OkgeError):                                    # table-shaped buffers are not row buffers
        hp.forward_backward(E, R, "complex", real, torch.empty_like(E), torch.empty_like(R), row_grads=True)
    with pytest.raises(N.OkgeError):
        hp.forward_backward(E, R, "complex", real, None, None, row_grads=True, loss_only=True)
    # a contiguous candidate range: rows first_id .. first_id + n - 1 are gathered, the result is the id-list call's
    rng_batch = H.PrefixBatch(po_rel=real.po_rel, po_obj=real.po_obj, sp_subj=real.sp_subj, sp_rel=real.sp_rel, pos_row=prow, pos_col=pcol,
                              cand_first=5, n_cand=n)
    lst_batch = H.PrefixBatch(po_rel=real.po_rel, po_obj=real.po_obj, sp_subj=real.sp_subj, sp_rel=real.sp_rel, pos_row=prow, pos_col=pcol,
                              cand_ids=torch.arange(5, 5 + n, dtype=torch.int32, device="cuda"))
    out = []
    for b in (rng_batch, lst_batch):
        gE, gR = torch.empty((n + 8, d), device="cuda"), torch.empty((8, d), device="cuda")
        loss = hp.forward_backward(E, R, "complex", b, gE, gR, row_grads=True).clone()
        out.append((loss, gE, gR))
    for a, b in zip(*out):
        assert torch.equal(a, b)
