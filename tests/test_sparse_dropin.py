"""The drop-in path with sparse gradients: AddLossModule(sparse_grads=True) hands autograd uncoalesced sparse gradients (one value
row per candidate / prefix occurrence, as the backward of nn.Embedding(sparse=True) does) and OkgeAdagrad(weight_decay=0) updates
the rows they name -- on the inputs of the reference's own sparse run (tests/golden/g21_sparse_*.npz)."""
import numpy as np
import pytest
import torch

from conftest import golden, golden_names
from open_knowledge_graph_embeddings_amd import hotpath as H
import sparse_reference as sr
from test_oracle_golden import adagrad_tol


def _dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dt is None else t.to(dt)).cuda()


def _model(z, name):
    from open_knowledge_graph_embeddings_amd.dataset import EntityRelationDatasetMeta
    from open_knowledge_graph_embeddings_amd.model import Models
    cls = "LookupComplexRelationModel" if "complex" in name else "LookupDistmultRelationModel"
    m = getattr(Models, cls)(entity_slot_size=z["E0"].shape[1], input_dropout=0.0, init_std=0.1, sparse=False,
                             train_data=EntityRelationDatasetMeta(entities_size=z["E0"].shape[0], relations_size=z["R0"].shape[0]))
    return m.cuda().train()


def _set(m, E, R):
    m.entity_embedding.weight.data.copy_(_dev(E))
    m.relation_embedding.weight.data.copy_(_dev(R))
    m.entity_embedding.weight.grad = m.relation_embedding.weight.grad = None


def _inputs(po_rel, po_obj, sp_subj, sp_rel, cand, labels):
    """(inputs, coordinate labels, candidate ids) as the batch producer emits them: int32, contiguous, on the device"""
    po = (_dev(po_rel, torch.int32), _dev(po_obj, torch.int32)) if len(po_rel) else None
    sp = (_dev(sp_subj, torch.int32), _dev(sp_rel, torch.int32)) if len(sp_subj) else None
    prow, pcol = H.positives_from_dense(_dev(labels))
    return [po, sp], (prow, pcol), _dev(cand, torch.int32)


def _golden_inputs(z, i):
    return _inputs(z[f"s{i}_po_rel"], z[f"s{i}_po_obj"], z[f"s{i}_sp_subj"], z[f"s{i}_sp_rel"], z[f"s{i}_cand"], z[f"s{i}_labels"])


def _backward(mod, inputs, labels, cand, normalizer):
    loss, hook, outs = mod(inputs=inputs, labels=labels, use_batch_shared_entities=True, batch_shared_entities=cand, epoch=1,
                           input_style_triple_or_prefix="right_and_left_prefix")
    assert hook is None and outs is None
    (loss.sum() / normalizer).backward()
    return loss.detach()


def _module(m, sparse_grads):
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule
    return AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0, training_outputs=False, sparse_grads=sparse_grads).train()


@pytest.mark.gpu
@pytest.mark.parametrize("name", golden_names("g21_sparse_"))
def test_sparse_gradients_are_the_dense_ones_uncoalesced(okge_lib, name):
    z = golden(name)
    m = _model(z, name)
    # the golden's first batch with its prefixes redrawn so that every row receives at most two contributions: torch's coalesce()
    # and the dense path's float atomics then add the same two numbers, in whatever order
    cand = z["s0_cand"]
    rest = np.setdiff1d(np.arange(2, z["E0"].shape[0]), cand)
    ent = np.array([cand[0], cand[1], rest[0], rest[0], rest[1], rest[1], rest[2], rest[3]], np.int32)
    rel = np.array([2, 2, 3, 3, 4, 4, 5, 6], np.int32)
    ids_e, ids_r = sr.occurrence_ids(cand, (rel[:4], ent[:4]), (ent[4:], rel[4:]))
    assert np.bincount(ids_e).max() == 2 and np.bincount(ids_r).max() == 2
    inputs, labels, cand_dev = _inputs(rel[:4], ent[:4], ent[4:], rel[4:], cand, z["s0_labels"])
    grads = {}
    for sparse_grads in (False, True):
        _set(m, z["E0"], z["R0"])
        loss = _backward(_module(m, sparse_grads), inputs, labels, cand_dev, float(z["s0_labels"].size))
        grads[sparse_grads] = (loss, m.entity_embedding.weight.grad, m.relation_embedding.weight.grad)
    assert torch.equal(grads[False][0], grads[True][0])
    for dense, sparse, ids in ((grads[False][1], grads[True][1], ids_e), (grads[False][2], grads[True][2], ids_r)):
        assert sparse.is_sparse and not dense.is_sparse and not sparse.is_coalesced() and sparse.shape == dense.shape
        assert sparse._indices().shape == (1, len(ids)) and np.array_equal(sparse._indices()[0].cpu().numpy(), ids)
        assert sparse._values().shape == (len(ids), dense.shape[1])
        assert torch.equal(sparse.coalesce().to_dense().view(torch.int32), dense.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", golden_names("g21_sparse_"))
def test_three_steps_reproduce_the_reference_and_the_fused_sparse_step(okge_lib, name):
    """each step restarted from the reference's state before it (a trajectory amplifies rounding noise through
    p -= lr * g / (|g| + eps), test_oracle_golden.py G3), within the G3 bound; bit-equal to FusedTrainStep(sparse=True)"""
    from open_knowledge_graph_embeddings_amd.optim import OkgeAdagrad
    from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep
    z = golden(name)
    scorer = "complex" if "complex" in name else "distmult"
    lr, eps = float(z["opt_lr"]), float(z["opt_eps"])
    m = _model(z, name)
    mod = _module(m, True)
    opt = OkgeAdagrad(m.parameters(), lr=lr, weight_decay=0, eps=eps)
    we, wr = m.entity_embedding.weight, m.relation_embedding.weight
    for i in range(int(z["nsteps"])):
        E, R = (z["E0"], z["R0"]) if i == 0 else (z[f"s{i-1}_E"], z[f"s{i-1}_R"])
        sE, sR = (np.zeros_like(E), np.zeros_like(R)) if i == 0 else (z[f"s{i-1}_sumE"], z[f"s{i-1}_sumR"])
        _set(m, E, R)
        opt.state[we]["sum"], opt.state[wr]["sum"] = _dev(sE), _dev(sR)
        inputs, labels, cand = _golden_inputs(z, i)
        loss = _backward(mod, inputs, labels, cand, float(z[f"s{i}_labels"].size))
        assert we.grad.is_sparse and wr.grad.is_sparse
        opt.step()
        assert abs(float(loss) - float(z[f"s{i}_loss"])) <= 3e-5 * abs(float(z[f"s{i}_loss"]))
        for mine, s_mine, ref, s_ref, s_prev in ((we, opt.state[we]["sum"], z[f"s{i}_E"], z[f"s{i}_sumE"], sE),
                                                 (wr, opt.state[wr]["sum"], z[f"s{i}_R"], z[f"s{i}_sumR"], sR)):
            got = mine.detach().cpu().numpy()
            tol = adagrad_tol(s_ref, s_prev, lr, eps)
            assert np.all(np.abs(got - ref) <= tol), float((np.abs(got - ref) / tol).max())
            np.testing.assert_allclose(np.sqrt(s_mine.cpu().numpy()), np.sqrt(s_ref), rtol=1e-4, atol=1e-6 * np.sqrt(s_ref.max()))
        # the same step by FusedTrainStep(sparse=True) from the same state
        st = FusedTrainStep(_dev(E), _dev(R), scorer, lr=lr, weight_decay=0.0, eps=eps, sparse=True)
        st.sumE.copy_(_dev(sE))
        st.sumR.copy_(_dev(sR))
        po, sp = inputs
        batch = H.PrefixBatch(po_rel=None if po is None else po[0], po_obj=None if po is None else po[1], sp_subj=sp[0], sp_rel=sp[1],
                              pos_row=labels[0], pos_col=labels[1], cand_ids=cand)
        fused_loss = st.step(batch)
        assert float(fused_loss.to(torch.float32)) == float(loss)
        for a, b in ((st.E, we.detach()), (st.R, wr.detach()), (st.sumE, opt.state[we]["sum"]), (st.sumR, opt.state[wr]["sum"])):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert float(opt.state[we]["step"]) == 3.0


@pytest.mark.gpu
def test_fast_call_and_general_path_agree(okge_lib, monkeypatch):
    from open_knowledge_graph_embeddings_amd import trainer
    z = golden("g21_sparse_complex")
    m = _model(z, "complex")
    out = {}
    for fast in (True, False):
        monkeypatch.setattr(trainer, "FAST_CALL", fast)
        _set(m, z["E0"], z["R0"])
        mod = _module(m, True)
        inputs, labels, cand = _golden_inputs(z, 0)
        loss = _backward(mod, inputs, labels, cand, float(z["s0_labels"].size))
        assert (getattr(mod, "_fd", None) is not None) == fast              # the persistent descriptors exist only on the fast call
        out[fast] = (loss, m.entity_embedding.weight.grad, m.relation_embedding.weight.grad)
    # ... and a non-contiguous id tensor sends the fast configuration down the general path
    monkeypatch.setattr(trainer, "FAST_CALL", True)
    _set(m, z["E0"], z["R0"])
    inputs, labels, cand = _golden_inputs(z, 0)
    wide = torch.stack([cand, cand], 1)[:, 0]
    assert not wide.is_contiguous()
    loss = _backward(_module(m, True), inputs, labels, wide, float(z["s0_labels"].size))
    out["strided"] = (loss, m.entity_embedding.weight.grad, m.relation_embedding.weight.grad)
    for other in (False, "strided"):
        assert torch.equal(out[True][0], out[other][0])
        for a, b in zip(out[True][1:], out[other][1:]):
            assert a.is_sparse and b.is_sparse and torch.equal(a._indices(), b._indices())
            assert torch.equal(a._values().view(torch.int32), b._values().view(torch.int32))


@pytest.mark.gpu
def test_upstream_scale_acts_on_the_value_rows(okge_lib):
    z = golden("g21_sparse_distmult")
    m = _model(z, "distmult")
    vals = []
    for normalizer in (float(z["s0_labels"].size), 50.0):
        _set(m, z["E0"], z["R0"])
        inputs, labels, cand = _golden_inputs(z, 0)
        _backward(_module(m, True), inputs, labels, cand, normalizer)
        vals.append(m.entity_embedding.weight.grad._values().clone())
    scale = np.float32(z["s0_labels"].size) / np.float32(50.0)
    np.testing.assert_allclose(vals[1].cpu().numpy(), vals[0].cpu().numpy() * scale, rtol=4e-7, atol=0)     # two fp32 roundings


@pytest.mark.gpu
def test_okge_adagrad_sparse_refusal_mixed_groups_and_lr_decay(okge_lib):
    from open_knowledge_graph_embeddings_amd.optim import OkgeAdagrad
    torch.manual_seed(0)
    p = torch.nn.Parameter(torch.randn(9, 8, device="cuda"))
    idx = torch.tensor([[1, 1, 7]], device="cuda")
    p.grad = torch.sparse_coo_tensor(idx, torch.randn(3, 8, device="cuda"), (9, 8))
    with pytest.raises(RuntimeError, match="weight_decay option is not compatible with sparse gradients"):
        OkgeAdagrad([p], lr=0.3, weight_decay=1e-10).step()
    # a mixed group (one sparse, one dense gradient) with lr_decay against torch.optim.Adagrad on the CPU, two steps
    q = torch.nn.Parameter(torch.randn(5, 8, device="cuda"))
    pc, qc = torch.nn.Parameter(p.detach().cpu().clone()), torch.nn.Parameter(q.detach().cpu().clone())
    mine = OkgeAdagrad([p, q], lr=0.3, lr_decay=0.5, weight_decay=0, eps=1e-8)
    ref = torch.optim.Adagrad([pc, qc], lr=0.3, lr_decay=0.5, weight_decay=0, eps=1e-8)
    for _ in range(2):
        v, gq = torch.randn(3, 8), torch.randn(5, 8)
        p.grad, q.grad = torch.sparse_coo_tensor(idx, v.cuda(), (9, 8)), gq.cuda()
        pc.grad, qc.grad = torch.sparse_coo_tensor(idx.cpu(), v, (9, 8)), gq.clone()
        mine.step()
        ref.step()
    for a, b in ((p, pc), (q, qc)):
        np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().numpy(), rtol=0, atol=3e-6)      # (the bound of the dense class test)
        np.testing.assert_allclose(mine.state[a]["sum"].cpu().numpy(), ref.state[b]["sum"].numpy(), rtol=1e-6, atol=1e-12)
    assert not mine.state[p]["sum"].is_sparse and mine.state[p]["sum"].shape == p.shape      # the state layout is torch's
    ref.load_state_dict(mine.state_dict())
