"""AddLossModule(fused_variants=True): the lookup embedder's variants on the HIP encode (csrc/okge_lookup_encode.hip through
lookup_variants.LookupVariantTrainStep) against G12 = the reference's LookupComplexRelationModel + AddLossModule -- the
assertions of test_embedder_variants.test_variant_forward_backward_matches_reference, line for line, at its tolerances, with
the torch encode patched to raise.  g12_variant_all_noshare (batch_shared_entities=None: one candidate block per direction)
keeps the torch fall-through in training with the keyword on."""
import numpy as np
import pytest
import torch

from conftest import golden
from test_embedder_variants import _model

pytestmark = pytest.mark.gpu

CASES = ["g12_variant_bn", "g12_variant_proj", "g12_variant_norm", "g12_variant_l2", "g12_variant_all"]


def _forbid_torch_encode(monkeypatch, m):
    def refuse(*args, **kwargs):
        raise AssertionError("the torch encode ran")
    monkeypatch.setattr(m, "_encode_torch", refuse)


def _run(z, m, mod, shared):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    inputs = [(t(z["po_rel"]), t(z["po_obj"])), (t(z["sp_subj"]), t(z["sp_rel"]))]
    return inputs, mod(inputs=inputs, labels=t(z["labels"]), use_batch_shared_entities=False, batch_shared_entities=shared, epoch=1,
                       input_style_triple_or_prefix="right_and_left_prefix")


@pytest.mark.parametrize("name", CASES)
def test_fused_variants_match_reference(okge_lib, monkeypatch, name):
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule
    z = golden(name)
    m = _model(z, cuda=True)
    m.train()
    mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0, fused_variants=True)
    _forbid_torch_encode(monkeypatch, m)
    shared = torch.from_numpy(np.ascontiguousarray(z["cand"])).cuda()
    inputs, (loss, hook, outs) = _run(z, m, mod, shared)
    np.testing.assert_allclose(outs.cpu().numpy(), z["outputs"], rtol=0, atol=1e-4)
    assert abs(float(loss.detach()) - float(z["loss"])) <= 3e-5 * abs(float(z["loss"]))
    assert (hook is not None) == bool(z["has_hook"])
    backward_loss = loss.sum()
    if hook is not None:
        assert abs(float(hook.detach()) - float(z["hook"])) <= 1e-5 * abs(float(z["hook"]))
        backward_loss = backward_loss + hook
    (backward_loss / float(z["normalizer"])).backward()                   # trainer.py:217-222
    for k, p in m.named_parameters():
        ref = z["g_" + k]
        got = p.grad.cpu().numpy() if p.grad is not None else np.zeros_like(ref)
        np.testing.assert_allclose(got, ref, rtol=0, atol=5e-5 * np.abs(ref).max() + 1e-10, err_msg=k)
    for k in z.files:
        if k.startswith("after_"):
            np.testing.assert_allclose(m.state_dict()[k[6:]].cpu().numpy(), z[k], rtol=1e-5, atol=1e-6, err_msg=k)
    m.eval()
    with torch.no_grad():
        _, (l2, h2, o2) = _run(z, m, mod, shared)
    # AddLossModule in eval mode scores BOTH directions against get_all_obj() (trainer.py:77-78); with an entity
    # projection the po rows therefore differ from po_prefix_score's (get_all_subj): compare what must agree
    n_po = z["po_rel"].shape[0]
    np.testing.assert_allclose(o2[n_po:].cpu().numpy(), z["eval_outputs"][n_po:], rtol=0, atol=1e-4)
    if not bool(z["project_entity"]):
        np.testing.assert_allclose(o2[:n_po].cpu().numpy(), z["eval_outputs"][:n_po], rtol=0, atol=1e-4)
    assert h2 is None and torch.isfinite(l2)
    if bool(z["batch_norm"]):                                             # eval mode moved no statistic
        for k in z.files:
            if k.startswith("after_"):
                np.testing.assert_allclose(m.state_dict()[k[6:]].cpu().numpy(), z[k], rtol=1e-5, atol=1e-6, err_msg=k)


def test_per_direction_candidates_keep_the_fall_through(okge_lib):
    """batch_shared_entities=None in training: two candidate blocks, the torch encode, the reference's numbers as before"""
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule
    z = golden("g12_variant_all_noshare")
    m = _model(z, cuda=True)
    m.train()
    calls = []
    encode_torch = m._encode_torch
    m._encode_torch = lambda *a, **k: (calls.append(1), encode_torch(*a, **k))[1]
    mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0, fused_variants=True)
    _, (loss, hook, outs) = _run(z, m, mod, None)
    assert len(calls) == 6                                                # (candidates, relation, entity) per direction
    np.testing.assert_allclose(outs.cpu().numpy(), z["outputs"], rtol=0, atol=1e-4)
    assert abs(float(loss.detach()) - float(z["loss"])) <= 3e-5 * abs(float(z["loss"]))
    assert abs(float(hook.detach()) - float(z["hook"])) <= 1e-5 * abs(float(z["hook"]))
    ((loss.sum() + hook) / float(z["normalizer"])).backward()
    for k, p in m.named_parameters():
        ref = z["g_" + k]
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=0, atol=5e-5 * np.abs(ref).max() + 1e-10, err_msg=k)


def test_keyword_refusals(okge_lib):
    from open_knowledge_graph_embeddings_amd.dataset import EntityRelationDatasetMeta
    from open_knowledge_graph_embeddings_amd.model import Models
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule
    data = EntityRelationDatasetMeta(entities_size=20, relations_size=5)
    loss = torch.nn.BCEWithLogitsLoss(reduction="sum")
    plain = Models.LookupComplexRelationModel(entity_slot_size=8, train_data=data)
    with pytest.raises(NotImplementedError, match="plain lookup model"):
        AddLossModule(plain, loss, 0.0, fused_variants=True)
    with pytest.raises(ValueError, match="FusedTrainStep"):
        plain.train_step()
    tanh = Models.LookupComplexRelationModel(entity_slot_size=8, train_data=data, project_entity=True, project_entity_activation="Tanh")
    with pytest.raises(NotImplementedError, match="ReLU"):
        AddLossModule(tanh, loss, 0.0, fused_variants=True)
    with pytest.raises(NotImplementedError, match="ReLU"):
        tanh.train_step()
    wide = Models.LookupComplexRelationModel(entity_slot_size=520, train_data=data, batch_norm=True)
    with pytest.raises(NotImplementedError, match="512"):
        wide.train_step()
    bn = Models.LookupComplexRelationModel(entity_slot_size=8, train_data=data, batch_norm=True)
    with pytest.raises(NotImplementedError, match="fused_l2_reg"):
        AddLossModule(bn, loss, 0.0, fused_variants=True, sparse_grads=True)
    # the wrappers around a step refuse the new one before they touch anything
    from open_knowledge_graph_embeddings_amd.sharded import ReplicaStep
    from open_knowledge_graph_embeddings_amd.train_step import GraphedTrainStep
    st = bn.cuda().train_step()
    with pytest.raises(NotImplementedError, match="eager steps on one device"):
        GraphedTrainStep(st, None, 16)
    with pytest.raises(NotImplementedError, match="eager steps on one device"):
        ReplicaStep(st)
