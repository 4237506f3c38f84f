"""DataBiasOnlyEntityModel / DataBiasOnlyRelationModel on the GPU against the reference's own models
(tests/golden/g20_databias_*.npz), written like test_lstm_parity.py and held to its bounds: scores rtol = atol = 1e-5, loss 1e-5
relative, gradients within 1e-4 of the tensor's largest element, running statistics rtol 1e-5 / atol 1e-6, Adagrad steps
restarted from the reference's state under that file's conditioning-aware bound.  Besides: the entity model's relation slot
stays bit-unchanged while its running statistics move, its parameters get no .grad through AddLossModule, the relation model's
padding row gets no gradient, and a second run is bit-identical."""
import numpy as np
import pytest
import torch

from conftest import golden, golden_names
from test_lstm_api import build
from test_lstm_parity import LSTM_KEYS, SIDES, close_to_largest, dev, grads_of, slots, sub

pytestmark = pytest.mark.gpu

CASES = [n for n in golden_names("g20_databias_") if "adagrad" not in n]
ADAGRAD = [n for n in golden_names("g20_databias_") if "adagrad" in n]
SCORER_OF = {"DataBiasOnlyRelationModel": "bias_relation", "DataBiasOnlyEntityModel": "bias_entity"}


def batch_of(z, pre=""):
    from open_knowledge_graph_embeddings_amd.hotpath import PrefixBatch, positives_from_dense
    b = PrefixBatch()
    b.po_rel, b.po_obj = dev(z[pre + "po_rel"].reshape(-1)), dev(z[pre + "po_obj"].reshape(-1))
    if pre + "sp_subj" in z.files:
        b.sp_subj, b.sp_rel = dev(z[pre + "sp_subj"].reshape(-1)), dev(z[pre + "sp_rel"].reshape(-1))
    b.cand_ids = dev(z[pre + "cand"].reshape(-1).astype(np.int32))
    b.pos_row, b.pos_col = positives_from_dense(dev(z[pre + "labels"]))
    return b


def inputs_of(z, pre=""):
    sp = (dev(z[pre + "sp_subj"]), dev(z[pre + "sp_rel"])) if pre + "sp_subj" in z.files else None
    return [(dev(z[pre + "po_rel"]), dev(z[pre + "po_obj"])), sp]


def check_running(z, e, r, prefix="buf/"):
    for side, sl in zip(SIDES, (e, r)):
        if sl.bn is not None:
            np.testing.assert_allclose(sl.running_mean.cpu().numpy(), z[f"{prefix}{side}_batchnorm.running_mean"], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(sl.running_var.cpu().numpy(), z[f"{prefix}{side}_batchnorm.running_var"], rtol=1e-5, atol=1e-6)


def slot_state(side, sl):
    """fixture name -> (parameter, accumulator)"""
    got = {f"{side}_embedding.weight": (sl.W, sl.sumW)}
    o = 0
    for k, t in zip(LSTM_KEYS, sl.lstm):
        got[f"{side}_encoder_in.{k}"] = (t, sl.sum_flat[o:o + t.numel()].view_as(t))
        o += t.numel()
    if sl.bn is not None:
        got[f"{side}_batchnorm.weight"] = (sl.bn[:sl.d], sl.sum_bn[:sl.d])
        got[f"{side}_batchnorm.bias"] = (sl.bn[sl.d:], sl.sum_bn[sl.d:])
    return got


@pytest.mark.parametrize("name", CASES)
def test_train_step_matches_reference(okge_lib, name):
    """LSTMTrainStep.forward_backward: loss, outputs, every gradient the reference has, running statistics of BOTH slots"""
    from open_knowledge_graph_embeddings_amd.lstm import LSTMTrainStep
    z = golden(name)
    scorer = SCORER_OF[str(z["model"])]
    e, r = slots(z, sub(z, "init/"))
    st = LSTMTrainStep(e, r, scorer, lr=0.1)
    B, N = z["labels"].shape
    scores = torch.empty((B, (N + 3) // 4 * 4), device="cuda:0")[:, :N]
    loss = st.forward_backward(batch_of(z), scores=scores)
    torch.cuda.synchronize()
    np.testing.assert_allclose(scores.cpu().numpy(), z["outputs"], rtol=1e-5, atol=1e-5)
    assert abs(float(loss[0]) - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
    mine = grads_of(st)
    none = {str(x) for x in z["grad_none"]}
    assert (scorer == "bias_entity") == bool(none)
    for k in (str(x) for x in z["param_names"]):
        if k in none:
            assert not mine[k].any(), k                          # the slot's backward did not run: its buffers are as made
        else:
            close_to_largest(mine[k], z["grad/" + k], 1e-4, k)
    assert not e.dW[0].any() and not r.dW[0].any()                 # padding_idx row: no gradient
    if scorer == "bias_relation":
        assert r.dW[1:].abs().sum() > 0 and e.dW[1:].abs().sum() > 0
    check_running(z, e, r)


@pytest.mark.parametrize("name", CASES)
def test_module_addloss_and_eval_match_reference(okge_lib, name):
    """the reference Trainer's statements on the seeded module: AddLossModule forward + backward (.grad, None where the
    reference's is None), then eval mode: precomputed tables and the prefix scores over all entities"""
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule
    z = golden(name)
    m = build(z).cuda()
    m.train()
    mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0)
    loss, _, outs = mod(inputs=inputs_of(z), labels=dev(z["labels"]), use_batch_shared_entities=bool(z["shared"]),
                        batch_shared_entities=dev(z["cand"]), epoch=1, input_style_triple_or_prefix="right_and_left_prefix")
    (loss.sum() / float(z["normalizer"])).backward()
    assert abs(float(loss.detach()) - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
    np.testing.assert_allclose(outs.detach().cpu().numpy(), z["outputs"], rtol=1e-5, atol=1e-5)
    none = {str(x) for x in z["grad_none"]}
    for k, p in m.named_parameters():
        if k in none:
            assert p.grad is None, k
        else:
            close_to_largest(p.grad, z["grad/" + k], 1e-4, k)
    for k, b in m.named_buffers():
        if "running" in k:
            np.testing.assert_allclose(b.cpu().numpy(), z["buf/" + k], rtol=1e-5, atol=1e-6, err_msg=k)
    m.eval()
    with torch.no_grad():
        m.precompute_embeddings_from_tokens()
        np.testing.assert_allclose(m.entity_embedding_from_tokens.cpu().numpy(), z["E_eval"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(m.relations_embedding_from_tokens.cpu().numpy(), z["R_eval"], rtol=1e-5, atol=1e-5)
        po = m.po_prefix_score(dev(z["po_rel"]), dev(z["po_obj"]))
        np.testing.assert_allclose(po.cpu().numpy(), z["po_all_eval"], rtol=1e-5, atol=1e-5)
        if int(z["has_sp"]):
            sp = m.sp_prefix_score(dev(z["sp_subj"]), dev(z["sp_rel"]))
            np.testing.assert_allclose(sp.cpu().numpy(), z["sp_all_eval"], rtol=1e-5, atol=1e-5)
        with pytest.raises(Exception):
            m(dev(z["po_obj"]), dev(z["po_rel"]), dev(z["po_obj"]))        # forward(subj, rel, obj): triple scoring raises


@pytest.mark.parametrize("name", ADAGRAD)
@pytest.mark.parametrize("step", [0, 1, 2])
def test_adagrad_steps_restarted_from_reference_state(okge_lib, name, step):
    """each of the reference's three OptimRegime Adagrad steps, restarted from the reference's state before it; parameters in
    `no_state` must come out bit-unchanged with untouched accumulators"""
    from open_knowledge_graph_embeddings_amd.lstm import LSTMTrainStep
    z = golden(name)
    pre, post = f"s{step}_before/", f"s{step}_after/"
    e, r = slots(z, sub(z, pre + "param/"), bufs=sub(z, pre + "buf/"), sums=sub(z, pre + "sum/"))
    st = LSTMTrainStep(e, r, SCORER_OF[str(z["model"])], lr=float(z["opt_lr"]), weight_decay=float(z["opt_weight_decay"]),
                       eps=float(z["opt_eps"]))
    B, N = z[f"s{step}_labels"].shape
    loss = st.step(batch_of(z, f"s{step}_"), normalizer=float(B * N))
    assert abs(float(loss[0]) - float(z[f"s{step}_loss"])) <= 1e-5 * abs(float(z[f"s{step}_loss"]))
    check_running(z, e, r, post + "buf/")
    no_state = {str(x) for x in z["no_state"]}
    lr, eps = float(z["opt_lr"]), float(z["opt_eps"])
    for side, sl in zip(SIDES, (e, r)):
        for k, (p, s) in slot_state(side, sl).items():
            want_p, want_s = z[post + "param/" + k], z[post + "sum/" + k]
            if k in no_state:
                np.testing.assert_array_equal(p.cpu().numpy(), z[pre + "param/" + k], err_msg=k)
                np.testing.assert_array_equal(p.cpu().numpy(), want_p, err_msg=k)
                assert not s.any(), k
                continue
            g = np.sqrt(want_s - z[pre + "sum/" + k])
            tol = 2e-4 * lr + lr * (1e-4 * g.max()) * (np.sqrt(z[pre + "sum/" + k]) + eps) / (np.sqrt(want_s) + eps) ** 2
            bad = np.abs(p.cpu().numpy() - want_p) > tol
            assert not bad.any(), (k, int(bad.sum()), float(np.abs(p.cpu().numpy() - want_p).max()))
            close_to_largest(s, want_s, 2e-4, k + " accumulator")


def test_entity_model_leaves_the_relation_slot_bit_unchanged(okge_lib):
    """three step() calls from the reference's initial state: every relation-slot parameter and accumulator torch.equal to its
    initial value (a zero-gradient Adagrad step would move a 0.3-sized weight by ~3e-4), the relation running statistics
    the fixture's after the third step"""
    from open_knowledge_graph_embeddings_amd.lstm import LSTMTrainStep
    z = golden("g20_databias_adagrad_entity")
    pre = "s0_before/"
    e, r = slots(z, sub(z, pre + "param/"), bufs=sub(z, pre + "buf/"), sums=sub(z, pre + "sum/"))
    before = {k: (p.clone(), s.clone()) for k, (p, s) in slot_state("relation", r).items()}
    d_before = [r.dW.clone(), r.d_flat.clone(), r.d_bn.clone()]
    st = LSTMTrainStep(e, r, "bias_entity", lr=float(z["opt_lr"]), weight_decay=float(z["opt_weight_decay"]), eps=float(z["opt_eps"]))
    for s in range(3):
        B, N = z[f"s{s}_labels"].shape
        st.step(batch_of(z, f"s{s}_"), normalizer=float(B * N))
    torch.cuda.synchronize()
    for k, (p, s) in slot_state("relation", r).items():
        assert torch.equal(p, before[k][0]) and torch.equal(s, before[k][1]), k
    for x, y in zip([r.dW, r.d_flat, r.d_bn], d_before):
        assert torch.equal(x, y)
    moved = max(float((r.running_mean - dev(z[pre + "buf/relation_batchnorm.running_mean"])).abs().max()),
                float((r.running_var - dev(z[pre + "buf/relation_batchnorm.running_var"])).abs().max()))
    assert moved > 1e-2
    for k in ("mean", "var"):
        np.testing.assert_allclose(getattr(r, "running_" + k).cpu().numpy(), z[f"s2_after/buf/relation_batchnorm.running_{k}"],
                                   rtol=1e-5, atol=1e-6)
    assert float((e.W - dev(z[pre + "param/entity_embedding.weight"])).abs().max()) > 0


def test_entity_model_without_batchnorm_skips_the_relation_encode(okge_lib, monkeypatch):
    """no batch-norm: nothing of the relation encode is observable, so the relation LSTM pass is not run at all"""
    from open_knowledge_graph_embeddings_amd import lstm as LM
    z = golden("g20_databias_entity_none_shared")
    e, r = slots(z, sub(z, "init/"))
    st = LM.LSTMTrainStep(e, r, "bias_entity")
    seen = []
    real = LM.LstmPass.encode
    monkeypatch.setattr(LM.LstmPass, "encode", lambda self, slot, *a, **k: (seen.append(slot), real(self, slot, *a, **k))[1])
    st.forward_backward(batch_of(z))
    torch.cuda.synchronize()
    assert seen == [e]


def test_addloss_with_torch_optimizer_skips_the_relation_parameters(okge_lib):
    """AddLossModule + torch's Adagrad over model.parameters(): the relation parameters' .grad is None, torch skips them, they
    stay bit-unchanged while every entity parameter moves"""
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule
    z = golden("g20_databias_adagrad_entity")
    m = build(z).cuda()
    m.train()
    mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0)
    opt = torch.optim.Adagrad(m.parameters(), lr=float(z["opt_lr"]), weight_decay=float(z["opt_weight_decay"]), eps=float(z["opt_eps"]))
    start = {k: p.detach().clone() for k, p in m.named_parameters()}
    for s in range(3):
        B, N = z[f"s{s}_labels"].shape
        opt.zero_grad()
        loss, _, _ = mod(inputs=inputs_of(z, f"s{s}_"), labels=dev(z[f"s{s}_labels"]), use_batch_shared_entities=True,
                         batch_shared_entities=dev(z[f"s{s}_cand"]), epoch=1, input_style_triple_or_prefix="right_and_left_prefix")
        (loss.sum() / float(B * N)).backward()
        for k, p in m.named_parameters():
            assert (p.grad is None) == k.startswith("relation_"), k
        opt.step()
    for k, p in m.named_parameters():
        if k.startswith("relation_"):
            assert torch.equal(p.detach(), start[k]), k
        else:
            assert not torch.equal(p.detach(), start[k]), k


def test_relation_model_padding_row_and_prefix_entities(okge_lib):
    """relation model: token row 0 gets no gradient in either slot; both slots learn"""
    from open_knowledge_graph_embeddings_amd.lstm import LSTMTrainStep
    z = golden("g20_databias_relation_bn_shared")
    e, r = slots(z, sub(z, "init/"))
    assert (dev(z["ent_tokens"]) == 0).any()
    st = LSTMTrainStep(e, r, "bias_relation")
    st.forward_backward(batch_of(z))
    torch.cuda.synchronize()
    assert not e.dW[0].any() and not r.dW[0].any()
    assert e.dW[1:].abs().sum() > 0 and r.dW[1:].abs().sum() > 0


@pytest.mark.parametrize("name", ["g20_databias_entity_bn_all", "g20_databias_relation_bn_shared"])
def test_bit_reproducible(okge_lib, name):
    from open_knowledge_graph_embeddings_amd.lstm import LSTMTrainStep
    z = golden(name)

    def run():
        e, r = slots(z, sub(z, "init/"))
        st = LSTMTrainStep(e, r, SCORER_OF[str(z["model"])], lr=0.1)
        losses = [float(st.step(batch_of(z))[0]) for _ in range(2)]
        torch.cuda.synchronize()
        return st, losses
    (a, la), (b, lb) = run(), run()
    assert la == lb
    for x, y in zip(a.state_tensors(), b.state_tensors()):
        assert torch.equal(x, y)
