"""Host-side refusals of the frozen-table feature (no GPU): every one of them is raised before a device, a process group or a
buffer is touched.  And the workspace: okge_train_workspace_bytes answers what it answered before the freeze flags existed (the
totals test_launch_plan.PINNED pinned from the planner at 256 compute units) -- a frozen call fits in the same workspace."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_launch_plan import KNOB_NAMES, PINNED  # noqa: E402


def _tables(d=8):
    return torch.zeros((12, d)), torch.zeros((5, d))


def test_flag_values():
    from open_knowledge_graph_embeddings_amd import _native as N
    from open_knowledge_graph_embeddings_amd import hotpath as H
    assert (N.OKGE_TRAIN_FREEZE_ENTITIES, N.OKGE_TRAIN_FREEZE_RELATIONS) == (64, 128)
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "okge.h")).read()
    assert "#define OKGE_TRAIN_FREEZE_ENTITIES 64" in header and "#define OKGE_TRAIN_FREEZE_RELATIONS 128" in header
    assert H.train_flags(grads_zero=True, freeze="entities") == 65 and H.train_flags(freeze="relations") == 128
    assert H.train_flags(grads_zero=True) == 1                                   # the default word is what it was
    with pytest.raises(ValueError, match="'entities' or 'relations'"):
        H.train_flags(freeze="both")


@pytest.mark.parametrize("kw,drop", [(dict(sparse=True, weight_decay=0.0), "sparse=True"), (dict(deterministic=True), "deterministic=True"),
                                     (dict(l2_reg=0.05), "l2_reg")])
@pytest.mark.parametrize("freeze", ["entities", "relations"])
def test_keyword_refusals_name_what_to_drop(freeze, kw, drop):
    from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep
    E, R = _tables()
    with pytest.raises(NotImplementedError, match="drop " + drop):
        FusedTrainStep(E, R, "complex", freeze=freeze, **kw)


@pytest.mark.parametrize("freeze", ["entity", "both", "E", True, 1])
def test_other_freeze_values_are_value_errors(freeze):
    from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep
    E, R = _tables()
    with pytest.raises(ValueError, match="freeze"):
        FusedTrainStep(E, R, "complex", freeze=freeze)


def test_multi_device_drivers_refuse():
    from open_knowledge_graph_embeddings_amd.sharded import ReplicaStep, ReplicaTrainStep, ShardedTrainStep
    E, R = _tables()
    with pytest.raises(NotImplementedError, match="ShardedTrainStep: freeze"):
        ShardedTrainStep(E, R, "complex", 12, freeze="entities")
    with pytest.raises(NotImplementedError, match="ReplicaTrainStep: freeze"):
        ReplicaTrainStep(E, R, "complex", freeze="relations")
    inner = types.SimpleNamespace(scorer="complex", freeze="entities")
    with pytest.raises(NotImplementedError, match="ReplicaStep: an inner step with a frozen table"):
        ReplicaStep(inner)


def test_freeze_param_naming_both_tables_of_a_bare_step():
    from open_knowledge_graph_embeddings_amd import checkpoint as C
    E, R = _tables()
    ckpt = {"state_dict": {C.ENTITY_KEY: E, C.RELATION_KEY: R}}
    called = []
    step = types.SimpleNamespace(E=E.clone(), R=R.clone(), set_freeze=called.append)
    for names in ([C.ENTITY_KEY, C.RELATION_KEY], ["True"]):
        with pytest.raises(ValueError, match="nothing is left to train"):
            C.load_reference_checkpoint(step, ckpt, freeze_param=names)
    assert not called
    assert C.freeze_names(None, [C.ENTITY_KEY]) == [] and C.freeze_names([], [C.ENTITY_KEY]) == []
    assert C.freeze_names([C.RELATION_KEY, "other.weight"], [C.ENTITY_KEY, C.RELATION_KEY]) == [C.RELATION_KEY]
    assert C.freeze_names("True", [C.ENTITY_KEY]) == []                          # (the reference looks at lists only)
    # a driver of the models that train every tensor they hold refuses a non-empty freeze_param before it reads anything
    with pytest.raises(NotImplementedError, match="trains every tensor it holds"):
        C.load_model_checkpoint(torch.nn.Linear(1, 1), object(), ckpt, freeze_param=[C.ENTITY_KEY])


def test_workspace_sizes_did_not_move(monkeypatch):
    from open_knowledge_graph_embeddings_amd import _native
    if _native.needs_build():
        _native.build_native()
    L = _native.lib()
    for name in KNOB_NAMES:
        monkeypatch.delenv("OKGE_" + name, raising=False)
    for (B, N, d), want in PINNED:
        assert L.okge_train_workspace_bytes(B, N, d) == want[-1], (B, N, d)
    assert np.int64(L.okge_train_workspace_bytes(65, 700, 1024)) > 0             # (the wide layout: pinned by test_wide_plan.py)
