"""lookup_variants.LookupVariantTrainStep as a training driver, on a small ComplEx model with all four `_encode` variants on:
three Adagrad steps, each against the float64 restatement (tests/lookup_variants_reference.py) + oracle.kge_oracle.adagrad_step
restarted from the step's own state (the G3 rule of test_hip_parity.test_g3_adagrad_steps / test_oracle_golden.adagrad_tol);
running statistics and num_batches_tracked against the module route (AddLossModule's torch fall-through + OkgeAdagrad) after the
same batches; checkpoint and resume, bit for bit, with Adagrad and with Adam; the clipped step's gradient norm."""
import numpy as np
import pytest
import torch

from lookup_variants_reference import FINAL_STREAMS, INPUT_STREAMS, default_cfg, full_step, philox_keeps
from oracle import kge_oracle as ko
from test_oracle_golden import adagrad_tol

pytestmark = pytest.mark.gpu

N_ENT, N_REL, D, N_PO, N_SP = 60, 8, 16, 6, 5
LR, WD, EPS = 0.1, 1e-10, 1e-8
DROPS = dict(dropout=0.2, relation_dropout=0.1, input_dropout=0.1, relation_input_dropout=0.15)
NO_DROPS = dict(dropout=0.0, relation_dropout=0.0, input_dropout=0.0, relation_input_dropout=0.0)
# the step's _param_groups() order under the restatement's names, and the module's parameter names
KEYS = ("E", "R", "bn_e_w", "bn_e_b", "bn_r_w", "bn_r_b", "W_subj", "W_obj")
RUNNING = (("bn_e_mean", "bn_e", "running_mean"), ("bn_e_var", "bn_e", "running_var"), ("bn_r_mean", "bn_r", "running_mean"),
           ("bn_r_var", "bn_r", "running_var"))


def build(seed=3, **drops):
    from open_knowledge_graph_embeddings_amd.dataset import EntityRelationDatasetMeta
    from open_knowledge_graph_embeddings_amd.model import Models
    torch.manual_seed(seed)
    m = Models.LookupComplexRelationModel(entity_slot_size=D, train_data=EntityRelationDatasetMeta(entities_size=N_ENT, relations_size=N_REL),
                                          batch_norm=True, project_entity=True, normalize="norm", l2_reg=0.01, init_std=0.3, seed=17,
                                          **drops)
    with torch.no_grad():                                    # batch-norm parameters off their trivial initial values
        for bn in (m.bn_e, m.bn_r):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0, 0.1)
    return m.cuda().train()


def batches(seed=11):
    """three batches: the candidate range, a sampled list, the range again -> [(PrefixBatch, ids dict, dense labels)]"""
    from open_knowledge_graph_embeddings_amd.hotpath import PrefixBatch, positives_from_dense
    rng = np.random.default_rng(seed)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    out = []
    for what in "ala":
        ids = {k: rng.integers(2, hi, n).astype(np.int32) for k, hi, n in (("po_rel", N_REL, N_PO), ("po_obj", N_ENT, N_PO),
                                                                          ("sp_subj", N_ENT, N_SP), ("sp_rel", N_REL, N_SP))}
        ids["cand"] = np.arange(2, N_ENT, dtype=np.int32) if what == "a" else rng.permutation(np.arange(2, N_ENT))[:24].astype(np.int32)
        b = PrefixBatch(**{k: dev(v) for k, v in ids.items() if k != "cand"})
        if what == "a":
            b.cand_first, b.n_cand = 2, N_ENT - 2
        else:
            b.cand_ids = dev(ids["cand"])
        y = np.zeros((N_PO + N_SP, len(ids["cand"])), np.float32)
        y[np.arange(N_PO + N_SP), rng.integers(0, len(ids["cand"]), N_PO + N_SP)] = 1
        b.pos_row, b.pos_col = positives_from_dense(dev(y))
        out.append((b, ids, y))
    return out


def snapshot(m, st):
    """the step's parameters, accumulators and running statistics as float64 arrays under the restatement's names"""
    groups = st._param_groups()
    P = {k: t[0].detach().cpu().double().numpy().copy() for k, t in zip(KEYS, groups)}
    S = {k: t[2].detach().cpu().double().numpy().copy() for k, t in zip(KEYS, groups)}
    for k, bn, name in RUNNING:
        P[k] = getattr(getattr(m, bn), name).detach().cpu().double().numpy().copy()
    return P, S


def test_three_adagrad_steps_against_float64(okge_lib):
    m = build(**DROPS)
    st = m.train_step(lr=LR, weight_decay=WD, eps=EPS)
    cfg = default_cfg(batch_norm=True, project=True, normalize="norm", l2_reg=0.01, **DROPS)
    for b, ids, y in batches():
        P, S = snapshot(m, st)
        step = st.steps + 1
        loss = st.step(b)
        torch.cuda.synchronize()
        want = full_step(ko.COMPLEX, P, cfg, ids, y, np.float64,
                         in_keeps=philox_keeps(17, step, D, ids, DROPS["input_dropout"], DROPS["relation_input_dropout"], INPUT_STREAMS),
                         out_keeps=philox_keeps(17, step, D, ids, DROPS["dropout"], DROPS["relation_dropout"], FINAL_STREAMS))
        assert abs(float(loss) - want["loss"]) <= 2e-5 * abs(want["loss"])
        P1, S1 = snapshot(m, st)
        for k in KEYS:
            p, s = P[k].copy(), S[k].copy()
            ko.adagrad_step(p, want["grads"][k], s, LR, WD, EPS)
            tol = adagrad_tol(s, S[k], LR, EPS)
            diff = np.abs(P1[k] - p)
            assert np.all(diff <= tol), (k, float((diff / tol).max()))
            assert np.mean(diff <= 2e-6) > 0.97, k
            np.testing.assert_allclose(np.sqrt(S1[k]), np.sqrt(s), rtol=1e-4, atol=1e-6 * np.sqrt(s.max()), err_msg=k)
            assert (P1[k] != P[k]).any(), f"{k} did not move"
        for k, _, _ in RUNNING:
            np.testing.assert_allclose(P1[k], want["running"][k], rtol=1e-5, atol=1e-6, err_msg=k)
        for t in st._param_groups():
            assert not t[1].any().item()                         # gradients cleared in the optimizer's sweep


def test_running_statistics_match_the_module_route(okge_lib):
    from open_knowledge_graph_embeddings_amd.optim import OkgeAdagrad
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule
    m1, m2 = build(**NO_DROPS), build(**NO_DROPS)
    st = m1.train_step(lr=LR, weight_decay=WD, eps=EPS)
    mod = AddLossModule(m2, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0)
    opt = OkgeAdagrad(m2.parameters(), lr=LR, weight_decay=WD, eps=EPS)
    for b, ids, y in batches():
        st.step(b)
        opt.zero_grad()
        loss, hook, _ = mod(inputs=[(b.po_rel, b.po_obj), (b.sp_subj, b.sp_rel)], labels=(b.pos_row, b.pos_col),
                            use_batch_shared_entities=True, batch_shared_entities=torch.from_numpy(ids["cand"]).cuda(), epoch=1,
                            input_style_triple_or_prefix="right_and_left_prefix")
        ((loss.sum() + hook) / float(y.size)).backward()
        opt.step()
    st.sync_module()
    for _, bn, name in RUNNING:
        np.testing.assert_allclose(getattr(getattr(m1, bn), name).cpu().numpy(), getattr(getattr(m2, bn), name).cpu().numpy(),
                                   rtol=1e-5, atol=1e-6, err_msg=f"{bn}.{name}")
    assert int(m1.bn_e.num_batches_tracked) == int(m2.bn_e.num_batches_tracked) == 9
    assert int(m1.bn_r.num_batches_tracked) == int(m2.bn_r.num_batches_tracked) == 6
    st.sync_module()                                             # (counted once)
    assert int(m1.bn_e.num_batches_tracked) == 9


@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
def test_checkpoint_and_resume_bit_for_bit(okge_lib, tmp_path, optimizer):
    from open_knowledge_graph_embeddings_amd import checkpoint as C
    kw = dict(lr=0.01 if optimizer == "adam" else LR, weight_decay=WD, eps=EPS, optimizer=optimizer, grad_clip=0.5)
    bs = batches()
    m1 = build(**DROPS)
    st1 = m1.train_step(**kw)
    for b, _, _ in bs:
        last1 = st1.step(b).clone()
    st1.sync_module()
    m2 = build(**DROPS)
    st2 = m2.train_step(**kw)
    for b, _, _ in bs[:2]:
        st2.step(b)
    path = str(tmp_path / "variants.pt")
    C.save_model_checkpoint(path, m2, st2, epoch=1)
    m3 = build(seed=99, **DROPS)
    st3 = m3.train_step(**kw)
    C.load_model_checkpoint(m3, st3, path)
    last3 = st3.step(bs[2][0]).clone()
    st3.sync_module()
    assert torch.equal(last1, last3)
    sd1, sd3 = m1.state_dict(), m3.state_dict()
    assert list(sd1) == list(sd3)
    for k in sd1:
        assert torch.equal(sd1[k], sd3[k]), k
    for a, b in zip(st1.state_tensors(), st3.state_tensors()):
        assert torch.equal(a, b)
    assert st1.steps == st3.steps == 3


def test_binding_grad_clip_reports_the_gradient_norm(okge_lib):
    m = build(**DROPS)
    st = m.train_step(lr=LR, weight_decay=WD, eps=EPS, grad_clip=1e-3)
    cfg = default_cfg(batch_norm=True, project=True, normalize="norm", l2_reg=0.01, **DROPS)
    b, ids, y = batches()[0]
    P, _ = snapshot(m, st)
    st.step(b)
    want = full_step(ko.COMPLEX, P, cfg, ids, y, np.float64,
                     in_keeps=philox_keeps(17, 1, D, ids, DROPS["input_dropout"], DROPS["relation_input_dropout"], INPUT_STREAMS),
                     out_keeps=philox_keeps(17, 1, D, ids, DROPS["dropout"], DROPS["relation_dropout"], FINAL_STREAMS))
    norm = np.sqrt(sum(float((want["grads"][k] ** 2).sum()) for k in KEYS))
    assert norm > 1e-3                                           # the clip binds
    assert abs(float(st.grad_norm) - norm) <= 1e-5 * norm
