"""The data-bias baseline models (DataBiasOnlyEntityModel / DataBiasOnlyRelationModel, openkge/model.py:281-350, :1036-1044):
the CPU-side surface against the reference's own constructor (tests/golden/g20_databias_*.npz) -- registry, MRO, seeded initial
parameters, state_dict keys, triple scoring raises, the step drivers that refuse the two scorers, the C header."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import golden, golden_names
from test_lstm_api import build

CASES = golden_names("g20_databias_")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIAS = ("bias_relation", "bias_entity")


def test_models_registered_with_the_reference_mro():
    import open_knowledge_graph_embeddings_amd  # noqa: F401
    from open_knowledge_graph_embeddings_amd.databias import DataBiasOnlyEntityScorer, DataBiasOnlyRelationScorer
    from open_knowledge_graph_embeddings_amd.lstm import LSTMRelationEmbedder
    from open_knowledge_graph_embeddings_amd.model import Models, RelationScorer
    for cls, scorer, name in ((Models.DataBiasOnlyEntityModel, DataBiasOnlyEntityScorer, "bias_entity"),
                              (Models.DataBiasOnlyRelationModel, DataBiasOnlyRelationScorer, "bias_relation")):
        assert cls.__mro__[1:4] == (scorer, RelationScorer, LSTMRelationEmbedder)      # model.py:1036-1044
        assert cls.scorer_name == name


def test_scorer_kinds_in_the_binding():
    from open_knowledge_graph_embeddings_amd import _native as N
    assert N.SCORERS["bias_relation"] == 2 and N.SCORERS["bias_entity"] == 3
    assert N.SCORERS["complex"] == 0 and N.SCORERS["distmult"] == 1


def test_header_carries_the_two_enum_values_at_abi_version_2():
    text = open(os.path.join(ROOT, "include", "okge.h")).read()
    assert re.search(r"#define\s+OKGE_ABI_VERSION\s+2\b", text)
    enum = re.search(r"enum\s+okge_scorer\s*\{(.*?)\};", text, re.S).group(1)
    assert re.search(r"OKGE_BIAS_RELATION\s*=\s*2\b", enum) and re.search(r"OKGE_BIAS_ENTITY\s*=\s*3\b", enum)
    assert "model.py:281-350" in enum


@pytest.mark.parametrize("name", CASES)
def test_seeded_construction_matches_reference(name):
    z = golden(name)
    m = build(z)
    assert [k for k, _ in m.named_parameters()] == [str(x) for x in z["param_names"]]
    for k, p in m.named_parameters():
        np.testing.assert_array_equal(p.detach().numpy(), z["init/" + k], err_msg=k)
    np.testing.assert_array_equal(m.entity_token_ids.numpy(), z["ent_tokens"])
    np.testing.assert_array_equal(m.relation_token_ids.numpy(), z["rel_tokens"])
    assert list(m.state_dict().keys()) == [str(x) for x in z["state_keys"]]


@pytest.mark.parametrize("name", ["g20_databias_entity_bn_all", "g20_databias_relation_bn_shared"])
def test_triple_scoring_raises(name):
    """model.py:311-312, :347-348: before anything is encoded or scored"""
    m = build(golden(name))
    rows = torch.zeros(3, int(golden(name)["d"]))
    with pytest.raises(Exception):
        m.triple_score(rows, rows, rows)
    with pytest.raises(Exception):
        m._score(rows, rows, rows, prefix=False)
    with pytest.raises(Exception):
        m._score(rows, rows, rows)


@pytest.mark.parametrize("scorer", BIAS)
def test_other_step_drivers_refuse(scorer):
    """every driver whose optimizer moves every parameter, and the sharded paths: NotImplementedError at construction, before
    a device, a process group or the library is touched"""
    from open_knowledge_graph_embeddings_amd.bigram import BigramTrainStep
    from open_knowledge_graph_embeddings_amd.sharded import ReplicaStep, ReplicaTrainStep, ShardedEvaluator, ShardedTrainStep
    from open_knowledge_graph_embeddings_amd.token_pooled import TokenPooledTrainStep
    from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep
    E, R = torch.zeros(8, 4), torch.zeros(4, 4)

    class Inner:
        pass
    inner = Inner()
    inner.scorer = scorer
    for make in (lambda: FusedTrainStep(E, R, scorer), lambda: ReplicaTrainStep(E, R, scorer),
                 lambda: ShardedTrainStep(E, R, scorer, 8), lambda: ShardedEvaluator(E, R, scorer, 8),
                 lambda: TokenPooledTrainStep(None, None, scorer), lambda: BigramTrainStep(None, None, scorer),
                 lambda: ReplicaStep(inner)):
        with pytest.raises(NotImplementedError, match=scorer):
            make()


def test_entity_model_keeps_relation_parameters_out_of_the_autograd_bridge():
    """autograd_params_and_grads: the parameters AddLossModule hands to autograd are the entity slot's only -- the fixture's
    `grad_none` names are exactly the ones left out"""
    z = golden("g20_databias_entity_bn_all")
    m = build(z)

    class Slot:
        d = int(z["d"])
        dW = torch.zeros(1)
        d_bn = torch.zeros(2 * int(z["d"]))
        dlstm = [torch.zeros(1)] * 4

    class Step:
        entity = relation = Slot()
    params, grads = m.autograd_params_and_grads(Step())
    assert len(params) == len(grads)
    handed = {id(p) for p in params}
    left_out = [k for k, p in m.named_parameters() if id(p) not in handed]
    assert left_out == [str(x) for x in z["grad_none"]]


@pytest.mark.parametrize("scorer", BIAS)
def test_c_abi_refusals_come_before_any_device_work(scorer):
    """okge_score_triples, okge_fold_queries, okge_evaluate_fused_shard: OKGE_ERR_UNSUPPORTED with a message
    naming the scorer, from the argument checks alone -- host buffers stand in for device memory, nothing reads or writes
    them (their sentinels stay), no device is needed.  An unknown scorer id is still OKGE_ERR_INVALID."""
    import ctypes
    from open_knowledge_graph_embeddings_amd import _native as N
    L = N.lib()
    kind = N.SCORERS[scorer]
    name = {"bias_relation": b"OKGE_BIAS_RELATION", "bias_entity": b"OKGE_BIAS_ENTITY"}[scorer]
    buf = np.full(4096, -7.0, np.float32)
    ids = np.full(64, 2, np.int32)
    p, q = buf.ctypes.data, ids.ctypes.data
    t = N.Tables()
    t.E, t.R, t.n_ent, t.n_rel, t.d, t.scorer = p, p, 10, 5, 12, kind
    pb = N.PrefixBatch()
    pb.po_rel = pb.po_obj = q
    pb.n_po = 3
    c = N.Candidates()
    c.first_id, c.n = 0, 5
    sh = N.Shard()
    sh.ent_lo, sh.ent_hi = 0, 10
    calls = {
        "okge_score_triples": lambda: L.okge_score_triples(kind, p, 12, p, 12, p, 12, 5, 12, p, None),
        "okge_fold_queries": lambda: L.okge_fold_queries(ctypes.byref(t), ctypes.byref(pb), p, 16, p, None),
        "okge_evaluate_fused_shard": lambda: L.okge_evaluate_fused_shard(1, ctypes.byref(t), ctypes.byref(sh), p, 16, 3, ctypes.byref(c), 5, q,
                                                                         None, 0, q, q, q, 3, p, p, p, buf.nbytes, None),
    }
    for entry, call in calls.items():
        assert call() == -2, entry                             # OKGE_ERR_UNSUPPORTED
        msg = L.okge_last_error()
        assert name in msg and entry.encode() in msg, msg
    assert L.okge_score_triples(7, p, 12, p, 12, p, 12, 5, 12, p, None) == -1
    assert (buf == -7.0).all() and (ids == 2).all()
