"""CPU checks of the row-sparse training step: the NumPy statement (tests/sparse_reference.py) against the reference's own
sparse run (tests/golden/g21_sparse_*.npz: nn.Embedding(sparse=True) + torch.optim.Adagrad, make_golden_sparse.py) and
against the project's oracle dense step at weight_decay = 0, and the refusals of the Python layers."""
import numpy as np
import pytest
import torch

from conftest import golden, golden_names
from oracle import kge_oracle as ko
import sparse_reference as sr
from test_oracle_golden import adagrad_tol


def _step_inputs(z, i):
    po = (z[f"s{i}_po_rel"], z[f"s{i}_po_obj"]) if len(z[f"s{i}_po_rel"]) else None
    sp = (z[f"s{i}_sp_subj"], z[f"s{i}_sp_rel"])
    return po, sp, z[f"s{i}_cand"], z[f"s{i}_labels"]


def _state_before(z, i):
    if i == 0:
        E, R = z["E0"].copy(), z["R0"].copy()
        return E, R, np.zeros_like(E), np.zeros_like(R)
    return z[f"s{i-1}_E"].copy(), z[f"s{i-1}_R"].copy(), z[f"s{i-1}_sumE"].copy(), z[f"s{i-1}_sumR"].copy()


@pytest.mark.parametrize("name", golden_names("g21_sparse_"))
def test_golden_has_the_cases_it_promises(name):
    z = golden(name)
    assert float(z["opt_weight_decay"]) == 0 and float(z["opt_eps"]) == 1e-8 and float(z["opt_lr"]) == 0.3
    assert float(z["ref_sparse_vs_dense_over_bound"]) <= 0.1      # the reference's own sparse-vs-dense gap: 10x inside the bound
    assert len(z["s1_po_rel"]) == 0 and len(z["s1_sp_rel"]) == 8   # one step with only sp rows
    for i in range(3):
        po, sp, cand, _ = _step_inputs(z, i)
        ids_e, _ = sr.occurrence_ids(cand, po, sp)
        assert len(cand) == 24 and len(np.unique(ids_e[24:])) < len(ids_e[24:])      # an entity repeats among the prefixes
        assert np.intersect1d(ids_e[24:], cand).size > 0                             # and a prefix entity is also a candidate


@pytest.mark.parametrize("name", golden_names("g21_sparse_"))
def test_numpy_statement_matches_reference_sparse_run(name):
    """each step restarted from the reference's state before it, within the G3 bound (torch's coalesce() sums in its own order)"""
    z = golden(name)
    kind = ko.COMPLEX if "complex" in name else ko.DISTMULT
    lr, eps = float(z["opt_lr"]), float(z["opt_eps"])
    for i in range(int(z["nsteps"])):
        E, R, sE, sR = _state_before(z, i)
        E_in, R_in, pE, pR = E.copy(), R.copy(), sE.copy(), sR.copy()
        po, sp, cand, labels = _step_inputs(z, i)
        out = sr.row_grads(kind, E, R, po, sp, cand, labels)
        assert abs(out["loss"] - float(z[f"s{i}_loss"])) <= 2e-5 * abs(float(z[f"s{i}_loss"]))
        sr.adagrad_rows(E, sE, out["ids_e"], out["gE"], lr, eps)
        sr.adagrad_rows(R, sR, out["ids_r"], out["gR"], lr, eps)
        for mine, ref, s_mine, s_ref, s_prev in ((E, z[f"s{i}_E"], sE, z[f"s{i}_sumE"], pE), (R, z[f"s{i}_R"], sR, z[f"s{i}_sumR"], pR)):
            tol = adagrad_tol(s_ref, s_prev, lr, eps)
            assert np.all(np.abs(mine - ref) <= tol), float((np.abs(mine - ref) / tol).max())
            np.testing.assert_allclose(np.sqrt(s_mine), np.sqrt(s_ref), rtol=1e-4, atol=1e-6 * np.sqrt(s_ref.max()))
        # rows no occurrence names: bit-unchanged, in the statement and in the reference
        for mine, ref, before, ids in ((E, z[f"s{i}_E"], E_in, out["ids_e"]), (R, z[f"s{i}_R"], R_in, out["ids_r"])):
            untouched = np.setdiff1d(np.arange(mine.shape[0]), ids)
            assert untouched.size and np.array_equal(mine[untouched], before[untouched]) and np.array_equal(ref[untouched], before[untouched])


@pytest.mark.parametrize("name", golden_names("g21_sparse_"))
def test_numpy_statement_is_the_oracle_dense_step_at_zero_weight_decay(name):
    """bit for bit, every row: the oracle's dense Adagrad fed the gradient coalesced in the stated order"""
    z = golden(name)
    kind = ko.COMPLEX if "complex" in name else ko.DISTMULT
    for i in range(int(z["nsteps"])):
        E, R, sE, sR = _state_before(z, i)
        if i == 0:
            sE[5:9] = 0.25                                        # (warm accumulators too)
        po, sp, cand, labels = _step_inputs(z, i)
        out = sr.row_grads(kind, E, R, po, sp, cand, labels)
        for p, s, ids, g in ((E, sE, out["ids_e"], out["gE"]), (R, sR, out["ids_r"], out["gR"])):
            dense, touched = sr.coalesce(ids, g, p.shape[0])
            assert not dense[~touched].any()
            pd, sd = p.copy(), s.copy()
            ko.adagrad_step(pd, dense, sd, 0.3, 0.0, 1e-8)
            ps, ss = p.copy(), s.copy()
            sr.adagrad_rows(ps, ss, ids, g, 0.3, 1e-8)
            assert np.array_equal(pd.view(np.uint32), ps.view(np.uint32)) and np.array_equal(sd.view(np.uint32), ss.view(np.uint32))


def test_coalesce_adds_in_ascending_position():
    g = np.array([[1e8], [1.0], [-1e8], [1.0]], np.float32)
    dense, touched = sr.coalesce([3, 3, 3, 1], g, 5)
    assert dense[3, 0] == np.float32(np.float32(np.float32(1e8) + np.float32(1.0)) + np.float32(-1e8)) == 0.0
    assert dense[1, 0] == 1.0 and touched.tolist() == [False, True, False, True, False]
    dense, touched = sr.coalesce([7, -1, 2], np.ones((3, 2), np.float32), 4)      # ids outside the table are skipped
    assert touched.tolist() == [False, False, True, False]


# ---- refusals of the Python layers (no GPU needed: they are raised before anything touches a device) ---------------------------
def test_fused_train_step_sparse_refusals():
    from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep
    E, R = torch.zeros(6, 4), torch.zeros(3, 4)
    with pytest.raises(ValueError, match="weight_decay option is not compatible with sparse gradients"):
        FusedTrainStep(E, R, "complex", sparse=True, engine=object())            # (the default weight_decay is 1e-10)
    with pytest.raises(NotImplementedError, match="grad_clip"):
        FusedTrainStep(E, R, "complex", weight_decay=0.0, sparse=True, grad_clip=1.0, engine=object())
    with pytest.raises(NotImplementedError, match="accumulate"):
        FusedTrainStep(E, R, "complex", weight_decay=0.0, sparse=True, accumulate=2, engine=object())
    st = FusedTrainStep(E, R, "distmult", weight_decay=0.0, sparse=True, engine=object())
    assert st.dE is None and st.dR is None
    assert [t.data_ptr() for t in st.state_tensors()] == [t.data_ptr() for t in (st.E, st.R, st.sumE, st.sumR)]


def _meta(n_ent, n_rel):
    from open_knowledge_graph_embeddings_amd.dataset import EntityRelationDatasetMeta
    return EntityRelationDatasetMeta(entities_size=n_ent, relations_size=n_rel, min_entities_size=2, min_relations_size=2)


def test_add_loss_module_sparse_grads_keyword():
    from open_knowledge_graph_embeddings_amd.model import Models
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule
    loss = torch.nn.BCEWithLogitsLoss(reduction="sum")
    m = Models.LookupComplexRelationModel(entity_slot_size=8, init_std=0.1, sparse=False, train_data=_meta(20, 5))
    assert AddLossModule(m, loss, 0.0, training_outputs=False, sparse_grads=True).sparse_grads
    assert not AddLossModule(m, loss).sparse_grads
    variant = Models.LookupComplexRelationModel(entity_slot_size=8, init_std=0.1, sparse=False, batch_norm=True, train_data=_meta(20, 5))
    with pytest.raises(NotImplementedError, match="sparse_grads"):
        AddLossModule(variant, loss, sparse_grads=True)
    # the constructors keep refusing model_config.sparse in this version
    with pytest.raises(NotImplementedError):
        Models.LookupComplexRelationModel(entity_slot_size=8, init_std=0.1, sparse=True, train_data=_meta(20, 5))


def test_okge_adagrad_refuses_weight_decay_with_a_sparse_gradient():
    """torch's own message (torch.optim.Adagrad: 'weight_decay option is not compatible with sparse gradients'), raised before
    any device work; without weight decay a CPU parameter is refused as every CPU parameter is"""
    from open_knowledge_graph_embeddings_amd.optim import OkgeAdagrad
    p = torch.nn.Parameter(torch.zeros(5, 4))
    p.grad = torch.sparse_coo_tensor(torch.tensor([[1, 1, 3]]), torch.ones(3, 4), (5, 4))
    with pytest.raises(RuntimeError, match="weight_decay option is not compatible with sparse gradients"):
        OkgeAdagrad([p], lr=0.1, weight_decay=1e-10).step()
    with pytest.raises(RuntimeError, match="on the GPU"):
        OkgeAdagrad([p], lr=0.1, weight_decay=0).step()
