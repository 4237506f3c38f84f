"""Token-pooled models (UnigramPoolingRelationEmbedder, openkge/model.py:715-796): the CPU-side surface against the
reference's own constructor (tests/golden/g9_unigram_init_*.npz) -- seeded initial parameters, parameter order, state_dict
keys, token-id matrices --, the place of the three token embedder families under TokenBasedRelationEmbedder, and the dropout
probabilities the model hands to its training steps."""
import numpy as np
import pytest
import torch

from conftest import golden, golden_names
from test_lstm_api import _unflat

CASES = golden_names("g9_unigram_init_")


def meta_of(z):
    from open_knowledge_graph_embeddings_amd.dataset import EntityRelationDatasetMeta
    return EntityRelationDatasetMeta(entities_size=int(z["n_ent"]), relations_size=int(z["n_rel"]),
                                     entity_tokens_size=int(z["vt_e"]), relation_tokens_size=int(z["vt_r"]),
                                     max_length=tuple(int(x) for x in z["max_len"]),
                                     entity_id_to_tokens_map=_unflat(z["ent_map"], z["ent_map_off"]),
                                     relation_id_to_tokens_map=_unflat(z["rel_map"], z["rel_map_off"]))


def build(z, **over):
    from open_knowledge_graph_embeddings_amd.model import Models
    kw = dict(entity_slot_size=int(z["d"]), relation_slot_size=int(z["d"]), train_data=meta_of(z), pool="sum", dropout=0.0, init_std=0.3,
              normalize=None if str(z["normalize"]) == "None" else str(z["normalize"]), sparse=False)
    kw.update(over)
    torch.manual_seed(int(z["seed"]))
    return getattr(Models, str(z["model"]))(**kw)


def test_the_four_cases_are_there():
    assert CASES == ["g9_unigram_init_" + n for n in ("complex_bn", "complex_none", "distmult_bn", "distmult_none")]


@pytest.mark.parametrize("name", CASES)
def test_seeded_construction_matches_reference(name):
    """same seed, same constructor order -> bit-identical initial parameters, in the reference's order and names"""
    z = golden(name)
    m = build(z)
    assert [k for k, _ in m.named_parameters()] == [str(x) for x in z["param_names"]]
    for k, p in m.named_parameters():
        np.testing.assert_array_equal(p.detach().numpy(), z["init/" + k], err_msg=k)
    np.testing.assert_array_equal(m.entity_token_ids.numpy(), z["ent_tokens"])
    np.testing.assert_array_equal(m.relation_token_ids.numpy(), z["rel_tokens"])


@pytest.mark.parametrize("name", CASES)
def test_state_dict_keys_match_reference(name):
    z = golden(name)
    assert list(build(z).state_dict().keys()) == [str(x) for x in z["state_keys"]]


def test_the_three_families_are_siblings():
    from open_knowledge_graph_embeddings_amd.bigram import BigramPoolingRelationEmbedder
    from open_knowledge_graph_embeddings_amd.lstm import LSTMRelationEmbedder
    from open_knowledge_graph_embeddings_amd.token_embedder import TokenBasedRelationEmbedder
    from open_knowledge_graph_embeddings_amd.token_encoder import TokenEncoderEmbedder
    from open_knowledge_graph_embeddings_amd.token_pooled import UnigramPoolingRelationEmbedder
    assert TokenBasedRelationEmbedder in UnigramPoolingRelationEmbedder.__bases__
    assert TokenBasedRelationEmbedder in TokenEncoderEmbedder.__bases__
    for cls in (LSTMRelationEmbedder, BigramPoolingRelationEmbedder):
        assert cls.__bases__ == (TokenEncoderEmbedder,)
        assert not issubclass(cls, UnigramPoolingRelationEmbedder)
    assert not issubclass(TokenEncoderEmbedder, UnigramPoolingRelationEmbedder)


@pytest.fixture
def host_engine(monkeypatch):
    """train_step() / autograd_step() build their step without a device: the engine is never called"""
    from open_knowledge_graph_embeddings_amd import _native as nv, hotpath
    if nv.needs_build():
        nv.build_native()
    monkeypatch.setattr(hotpath, "HotPath", lambda device: object())


@pytest.mark.parametrize("relation_dropout,expected", [(0.4, 0.4), (None, 0.1)])
def test_steps_get_both_dropout_probabilities(host_engine, relation_dropout, expected):
    """the relation rows are masked with relation_dropout (model.py:755-758, :794-795), not with the entity probability"""
    m = build(golden("g9_unigram_init_complex_bn"), dropout=0.1, relation_dropout=relation_dropout)
    for st in (m.train_step(), m.autograd_step("bce", 0.0)):
        assert st.dropout == 0.1 and st.relation_dropout == expected
