"""The drop-in path with a frozen table (the reference's resume_freeze, trainer.py:532-536): AddLossModule reads requires_grad of
entity_embedding.weight / relation_embedding.weight on every call and passes OKGE_TRAIN_FREEZE_ENTITIES / _RELATIONS; the frozen
parameter gets no gradient (its .grad stays None) and OkgeAdagrad / OkgeAdam skip it as torch's optimizers do -- no decay, no
state change.  With sparse_grads=True or the fused l2_reg hook a frozen table keeps the full step (autograd drops its gradient).
Tolerance of the updated table: the 2e-6 of test_dropin_path.test_addloss_without_training_outputs_and_okge_adagrad_step."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_n3_step import _problems, dev  # noqa: E402

pytestmark = pytest.mark.gpu
D, N_ENT, N_REL, N_PO, N_SP, N_CAND = 300, 420, 90, 20, 17, 200      # slot size 300: the stream-K tile launch and its dc_reduce
KEYS = {"entities": "entity_embedding.weight", "relations": "relation_embedding.weight"}
# the launches that exist only for the entity table's candidate gradient, by the names okge_timing_* reports them under
DE_LAUNCHES = ("dc_reduce", "wide_dc_gemm", "wide_dc_scatter")


def _model(E, R, scorer="complex", **kw):
    from open_knowledge_graph_embeddings_amd.dataset import EntityRelationDatasetMeta
    from open_knowledge_graph_embeddings_amd.model import Models
    name = "LookupComplexRelationModel" if scorer == "complex" else "LookupDistmultRelationModel"
    m = getattr(Models, name)(entity_slot_size=E.shape[1], input_dropout=0.0, init_std=0.1, sparse=False, **kw,
                              train_data=EntityRelationDatasetMeta(entities_size=E.shape[0], relations_size=R.shape[0])).cuda()
    m.entity_embedding.weight.data.copy_(dev(E))
    m.relation_embedding.weight.data.copy_(dev(R))
    return m.train()


def _optimizer(m, name):
    from open_knowledge_graph_embeddings_amd.optim import OkgeAdagrad, OkgeAdam
    if name == "adam":
        return OkgeAdam(m.parameters(), lr=1e-2, weight_decay=1e-10)
    opt = OkgeAdagrad(torch.optim.Adam(m.parameters(), lr=0).param_groups)          # as OptimRegime.adjust does
    for grp in opt.param_groups:
        grp["lr"], grp["weight_decay"] = 0.3, 1e-10
    return opt


def _forward(mod, prob, fast):
    """fast: coordinate labels and int32 device ids (AddLossModule's persistent-struct call); else the general path on dense labels"""
    b, po, sp, cand, y = prob
    col = lambda a: dev(np.asarray(a, np.int32).reshape(-1, 1))       # noqa: E731
    labels = (b.pos_row, b.pos_col) if fast else dev(y)
    return mod(inputs=[(col(po[0]), col(po[1])), (col(sp[0]), col(sp[1]))], labels=labels, use_batch_shared_entities=True,
               batch_shared_entities=col(cand), epoch=1, input_style_triple_or_prefix="right_and_left_prefix")


def _timed_names(eng, fn):
    eng.timing(True)
    out = fn()
    torch.cuda.synchronize()
    names = set(eng.timing_collect())
    eng.timing(False)
    return out, names


@pytest.mark.parametrize("fast", [False, True], ids=["general", "fast"])
@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
@pytest.mark.parametrize("freeze", ["entities", "relations"])
def test_frozen_parameter_through_addloss_and_the_okge_optimizers(okge_lib, freeze, optimizer, fast):
    from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule
    E, R, probs = _problems(1, D, N_ENT, N_REL, N_PO, N_SP, seed=21, once=True, n_cand=N_CAND)
    m = _model(E, R)
    frozen_p = m.entity_embedding.weight if freeze == "entities" else m.relation_embedding.weight
    trained_p = m.relation_embedding.weight if freeze == "entities" else m.entity_embedding.weight
    mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0, training_outputs=False)
    eng = m.engine()
    # the unfrozen call first: it does launch what the frozen-entities call must not (the check below is not vacuous)
    (loss_u, _, _), names_u = _timed_names(eng, lambda: _forward(mod, probs[0], fast))
    assert "fused_tile_train" in names_u and "dc_reduce" in names_u, names_u
    opt = _optimizer(m, optimizer)
    frozen_p.requires_grad_(False)
    state0 = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state[frozen_p].items()}
    (loss, hook, outs), names = _timed_names(eng, lambda: _forward(mod, probs[0], fast))
    assert hook is None and outs is None and "fused_tile_train" in names and "prefix_backward" in names
    if freeze == "entities":
        assert not names & set(DE_LAUNCHES), names
    else:
        assert "dc_reduce" in names
    assert float(loss.detach()) == float(loss_u.detach())
    (loss.sum() / float((N_PO + N_SP) * N_CAND)).backward()
    assert frozen_p.grad is None and trained_p.grad is not None
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(frozen_p.data, dev(E if freeze == "entities" else R))
    assert set(opt.state[frozen_p]) == set(state0)
    for k, v in state0.items():
        assert torch.equal(opt.state[frozen_p][k], v) if torch.is_tensor(v) else opt.state[frozen_p][k] == v, k
    ts = FusedTrainStep(dev(E.copy()), dev(R.copy()), "complex", optimizer=optimizer, lr=1e-2 if optimizer == "adam" else 0.3,
                        weight_decay=1e-10, freeze=freeze)
    ts.step(probs[0][0])
    torch.cuda.synchronize()
    want = ts.R if freeze == "entities" else ts.E
    assert not torch.equal(want, dev(R if freeze == "entities" else E))              # (the step did train it)
    np.testing.assert_allclose(trained_p.detach().cpu().numpy(), want.cpu().numpy(), rtol=0, atol=2e-6)


@pytest.mark.parametrize("fast", [False, True], ids=["general", "fast"])
@pytest.mark.parametrize("variant", ["sparse_grads", "l2_reg"])
@pytest.mark.parametrize("freeze", ["entities", "relations"])
def test_frozen_parameter_with_sparse_grads_or_the_l2_reg_hook(okge_lib, freeze, variant, fast):
    """AddLossModule(sparse_grads=True) and the fused l2_reg hook keep the route they always took when one table is frozen: the
    occurrence-row call and the N3 kernel are not built for a missing buffer, so the whole step runs and autograd drops the
    gradient of the input that does not require one.  The frozen parameter's .grad is None, its data does not move, and the
    trained table is the one an unfrozen module gets from the same state"""
    from open_knowledge_graph_embeddings_amd.optim import OkgeAdagrad
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule
    E, R, probs = _problems(1, 24, 300, 80, 9, 8, seed=24, once=True, n_cand=100)
    norm = float(17 * 100)
    tables = {}
    for frozen in (True, False):
        m = _model(E, R, **(dict(l2_reg=0.05) if variant == "l2_reg" else {}))
        kw = dict(sparse_grads=True) if variant == "sparse_grads" else dict(fused_l2_reg=True)
        mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0, training_outputs=False, **kw)
        opt = OkgeAdagrad(m.parameters(), lr=0.3, weight_decay=0 if variant == "sparse_grads" else 1e-10, eps=1e-8)
        frozen_p = m.entity_embedding.weight if freeze == "entities" else m.relation_embedding.weight
        trained_p = m.relation_embedding.weight if freeze == "entities" else m.entity_embedding.weight
        if frozen:
            frozen_p.requires_grad_(False)
        loss, hook, _ = _forward(mod, probs[0], fast)
        assert (hook is not None) == (variant == "l2_reg")
        ((loss.sum() + (hook if hook is not None else 0.0)) / norm).backward()
        assert trained_p.grad is not None and trained_p.grad.is_sparse == (variant == "sparse_grads")
        if frozen:
            assert frozen_p.grad is None
        opt.step()
        torch.cuda.synchronize()
        if frozen:
            assert torch.equal(frozen_p.data, dev(E if freeze == "entities" else R))
        tables[frozen] = (float(loss.detach()), trained_p.detach().clone())
    assert tables[True][0] == tables[False][0]
    assert not torch.equal(tables[True][1], dev(R if freeze == "entities" else E))      # (it was trained)
    np.testing.assert_allclose(tables[True][1].cpu().numpy(), tables[False][1].cpu().numpy(), rtol=0, atol=2e-6)


def test_both_frozen_takes_the_loss_only_route(okge_lib):
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule
    E, R, probs = _problems(1, 24, 300, 80, 9, 8, seed=22, once=True, n_cand=100)
    m = _model(E, R)
    mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0, training_outputs=False)
    want = float(_forward(mod, probs[0], True)[0].detach())
    for p in m.parameters():
        p.requires_grad_(False)
    for fast in (False, True):
        (loss, _, _), names = _timed_names(m.engine(), lambda: _forward(mod, probs[0], fast))
        assert not loss.requires_grad and float(loss) == want
        assert "loss_reduce" in names and "prefix_backward" not in names and "dq" not in names, names


def test_load_model_checkpoint_freezes_the_named_parameters(okge_lib, tmp_path):
    from open_knowledge_graph_embeddings_amd import checkpoint as C
    from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep
    E, R, _ = _problems(1, 24, 60, 9, 2, 2, seed=23)
    path = str(tmp_path / "tables.pt")
    C.save_checkpoint(path, FusedTrainStep(dev(E), dev(R), "complex"))
    m = _model(np.zeros_like(E), np.zeros_like(R))
    C.load_model_checkpoint(m, None, path, freeze_param=[KEYS["entities"]])
    assert not m.entity_embedding.weight.requires_grad and m.relation_embedding.weight.requires_grad
    assert torch.equal(m.entity_embedding.weight.data, dev(E)) and torch.equal(m.relation_embedding.weight.data, dev(R))
    m2 = _model(np.zeros_like(E), np.zeros_like(R))
    C.load_model_checkpoint(m2, None, path, freeze_param=["True"])          # the reference's "all loaded names"
    assert not any(p.requires_grad for p in m2.parameters())
    m3 = _model(np.zeros_like(E), np.zeros_like(R))
    C.load_model_checkpoint(m3, None, path)
    assert all(p.requires_grad for p in m3.parameters())
