"""The float64 restatement of an LSTM pass (tests/lstm_reference.py) pinned to the reference's own LSTM{Complex,Distmult}
RelationModel on the CPU (tests/golden/g17_lstm_*.npz): the training-mode pass over the reference's call order reproduces its
running statistics, and the eval-mode pass over all ids its precomputed tables.  The GPU shape sweep (test_lstm_shapes.py)
holds the HIP kernels to this restatement."""
import numpy as np
import pytest
import torch

from conftest import golden, golden_names
from lstm_reference import lstm_pass

CASES = [n for n in golden_names("g17_lstm_") if n != "g17_lstm_adagrad"]
LSTM_KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def _slot(z, side):
    p = lambda k: torch.from_numpy(z[f"init/{side}_{k}"])                 # noqa: E731
    lstm = [p(f"encoder_in.{k}") for k in LSTM_KEYS]
    bn = (p("batchnorm.weight"), p("batchnorm.bias")) if f"init/{side}_batchnorm.weight" in z.files else None
    return p("embedding.weight"), lstm, bn


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_reference_running_stats_and_eval_tables(name):
    """entity slot: candidates (encoded once, AddLossModule -> precompute_batch_shared_inputs, in the "all" cases too), then
    po objects, then sp subjects; relation slot: po relations, then sp relations.  Then eval mode over every id."""
    z = golden(name)
    assert int(z["max_len"]) == z["ent_tokens"].shape[1]
    for side, tok, calls, n_all, table in (
            ("entity", "ent_tokens", ("cand", "po_obj", "sp_subj"), z["ent_tokens"].shape[0], "E_eval"),
            ("relation", "rel_tokens", ("po_rel", "sp_rel"), z["rel_tokens"].shape[0], "R_eval")):
        W, lstm, bn = _slot(z, side)
        tok = torch.from_numpy(z[tok])
        running = None
        if bn is not None:
            ids = [torch.from_numpy(z[c].reshape(-1).astype(np.int64)) for c in calls]
            tr = lstm_pass(W, tok, lstm, [(x, 0, x.numel()) for x in ids], bn=bn, training=True)
            np.testing.assert_allclose(tr["running_mean"], z[f"buf/{side}_batchnorm.running_mean"], rtol=1e-5, atol=1e-6,
                                       err_msg=side)
            np.testing.assert_allclose(tr["running_var"], z[f"buf/{side}_batchnorm.running_var"], rtol=1e-5, atol=1e-6,
                                       err_msg=side)
            running = (torch.from_numpy(tr["running_mean"]), torch.from_numpy(tr["running_var"]))
        ev = lstm_pass(W, tok, lstm, [(None, 0, n_all)], bn=bn, running=running, training=False)
        np.testing.assert_allclose(ev["out"], z[table], rtol=1e-5, atol=1e-5, err_msg=side)


def test_restatement_gradients_match_autograd_of_the_module():
    """the restatement's gradients (one training-mode call with batch-norm) are torch autograd's through the reference module's
    own op sequence (embedding -> nn.LSTM -> h at last -> BatchNorm1d), and the padding row gets none"""
    from test_lstm_api import build
    z = golden("g17_lstm_distmult_bn_shared")
    m = build(z).double()
    m.train()
    ids = torch.from_numpy(z["sp_subj"].reshape(-1).astype(np.int64))
    tokens = m.entity_token_ids[ids].long()
    h, _ = m.entity_encoder_in(m.entity_embedding(tokens))
    enc = m.entity_batchnorm(h[torch.arange(len(ids)), (tokens > 0).long().sum(1) - 1])
    w = torch.linspace(-1, 1, enc.numel(), dtype=torch.float64).reshape(enc.shape)
    (enc * w).sum().backward()
    W, lstm, bn = _slot(z, "entity")
    r = lstm_pass(W, m.entity_token_ids, lstm, [(ids, 0, len(ids))], bn=bn, training=True, d_out=w)
    np.testing.assert_allclose(r["out"], enc.detach().numpy(), rtol=1e-12, atol=1e-12)
    mods = [m.entity_embedding.weight] + [getattr(m.entity_encoder_in, k) for k in LSTM_KEYS] + \
        [m.entity_batchnorm.weight, m.entity_batchnorm.bias]
    for k, p in zip(("dW", "dW_ih", "dW_hh", "db_ih", "db_hh", "d_bn_weight", "d_bn_bias"), mods):
        np.testing.assert_allclose(r[k], p.grad.numpy(), rtol=1e-10, atol=1e-12, err_msg=k)
    assert not r["dW"][0].any()
