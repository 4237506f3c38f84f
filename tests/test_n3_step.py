"""The l2_reg hook (N3 regulariser, openkge/model.py:444-453, :471-479) through the Python drivers: AddLossModule(fused_l2_reg=True)
against what the unmodified reference computed (G12 `l2`, G23), and FusedTrainStep(l2_reg=...) -- dense, wide, row-sparse and
under GraphedTrainStep -- against the float64 restatement (tests/n3_reference.py) + the oracle's Adagrad."""
import numpy as np
import pytest
import torch

import n3_reference as nr
from conftest import golden, golden_names
from oracle import kge_oracle as ko

pytestmark = pytest.mark.gpu
FIXTURES = ["g12_variant_l2"] + golden_names("g23_n3_")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _model(f):
    from open_knowledge_graph_embeddings_amd.dataset import EntityRelationDatasetMeta
    from open_knowledge_graph_embeddings_amd.model import Models
    cls = Models.LookupComplexRelationModel if f["kind"] == "complex" else Models.LookupDistmultRelationModel
    m = cls(entity_slot_size=f["E"].shape[1], input_dropout=f["input_dropout"], dropout=f["dropout"], init_std=0.3, sparse=False,
            l2_reg=f["l2_reg"], train_data=EntityRelationDatasetMeta(entities_size=f["E"].shape[0], relations_size=f["R"].shape[0]))
    m.load_state_dict({"entity_embedding.weight": torch.from_numpy(f["E"]), "relation_embedding.weight": torch.from_numpy(f["R"])})
    return m.cuda().train()


def _replay_masks(m, f):
    """the captured Bernoulli masks of the reference in place of the model's Philox streams"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    by_stream = {H.STREAM_CAND: "keep_cand", H.STREAM_PO_ENT: "keep_po_ent", H.STREAM_SP_ENT: "keep_sp_ent"}
    keeps = {s: dev(f["keeps"][k].astype(np.uint8)) for s, k in by_stream.items() if k in f["keeps"]}

    def dropout_spec(stream, relation=False):
        if relation or stream not in keeps:
            return H.DropoutSpec()
        return H.DropoutSpec(p=f["p_ent"], keep=keeps[stream])
    m.dropout_spec = dropout_spec


# (the fast call draws its own masks: the dropout case, which replays the reference's, stays with the general path)
ROUTES = [(n, False) for n in FIXTURES] + [(n, True) for n in FIXTURES if not n.endswith("dropout")]


@pytest.mark.parametrize("name,fast", ROUTES, ids=[f"{n}-{'fast_call' if f else 'general'}" for n, f in ROUTES])
def test_fused_route_meets_the_fall_through_routes_bounds(okge_lib, name, fast):
    """outputs 1e-4, loss 3e-5, hook 1e-5, gradients 5e-5 of their largest (test_embedder_variants.py); `fast_call`: coordinate
    labels and int32 ids, the call with persistent structs"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule
    f = nr.fixture_problem(golden(name))
    assert not (fast and f["keeps"])
    m = _model(f)
    assert m.encode_in_torch
    if f["keeps"]:
        _replay_masks(m, f)
    mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0, fused_l2_reg=True)
    inputs = [None if p is None else (dev(p[0].astype(np.int32)), dev(p[1].astype(np.int32))) for p in (f["po"], f["sp"])]
    labels = H.positives_from_dense(dev(f["labels"])) if fast else dev(f["labels"])
    shared_list = name.endswith("repeat")
    shared = None if f["no_shared"] else dev(f["cand"].astype(np.int32))
    loss, hook, outs = mod(inputs=inputs, labels=labels, use_batch_shared_entities=shared_list, batch_shared_entities=shared, epoch=1,
                           input_style_triple_or_prefix="right_and_left_prefix")
    assert hook is not None and hook.requires_grad and hook.dtype == torch.float32
    print(f"{name}: loss {float(loss.detach()):.8g} vs {f['loss']:.8g}, hook {float(hook.detach()):.8g} vs {f['hook']:.8g}")
    np.testing.assert_allclose(outs.detach().cpu().numpy(), f["outputs"], rtol=0, atol=1e-4)
    assert abs(float(loss.detach()) - f["loss"]) <= 3e-5 * abs(f["loss"])
    assert abs(float(hook.detach()) - f["hook"]) <= 1e-5 * abs(f["hook"])
    ((loss.sum() + hook) / f["normalizer"]).backward()                   # trainer.py:217-222, unchanged
    for p, ref, k in ((m.entity_embedding.weight, f["dE"], "dE"), (m.relation_embedding.weight, f["dR"], "dR")):
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=0, atol=5e-5 * np.abs(ref).max() + 1e-10, err_msg=k)
    # no gradient, training mode: the hook's value alone; eval mode: no hook (model.py:471)
    with torch.no_grad():
        l2, h2, _ = mod(inputs=inputs, labels=labels, use_batch_shared_entities=shared_list, batch_shared_entities=shared, epoch=1,
                        input_style_triple_or_prefix="right_and_left_prefix")
    assert abs(float(h2) - f["hook"]) <= 1e-5 * abs(f["hook"]) and abs(float(l2) - f["loss"]) <= 3e-5 * abs(f["loss"])
    m.eval()
    with torch.no_grad():
        _, h3, _ = mod(inputs=inputs, labels=labels, use_batch_shared_entities=shared_list, batch_shared_entities=shared, epoch=1,
                       input_style_triple_or_prefix="right_and_left_prefix")
    assert h3 is None


# ---------------------------------------------------------------------------------------------------------- FusedTrainStep
def _problems(k, d, n_ent, n_rel, n_po, n_sp, seed, once=False, n_cand=None):
    """k batches on one pair of tables: 1-vs-all, or (n_cand) a unique sampled list.  once: every entity and every relation is
    named ONCE per batch -- prefix ids distinct, no prefix entity a candidate -- which leaves every float atomic of the step one
    addend per call onto a row nobody else adds to: order-free"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    rng = np.random.default_rng(seed)
    E, R = (rng.standard_normal((n_ent, d)) * 0.1).astype(np.float32), (rng.standard_normal((n_rel, d)) * 0.1).astype(np.float32)
    out, B = [], n_po + n_sp
    for _ in range(k):
        perm = rng.permutation(np.arange(2, n_ent))
        cand = np.arange(2, n_ent) if n_cand is None else perm[:n_cand]
        if once:
            ent, rel = perm[n_cand:n_cand + B].astype(np.int32), rng.permutation(np.arange(2, n_rel))[:B].astype(np.int32)
        else:
            ent, rel = rng.integers(2, n_ent, B).astype(np.int32), rng.integers(2, n_rel, B).astype(np.int32)
        po, sp = (rel[:n_po], ent[:n_po]), (ent[n_po:], rel[n_po:])
        y = np.zeros((B, len(cand)), np.float32)
        for r in range(B):
            y[r, rng.choice(len(cand), size=int(rng.integers(1, 4)), replace=False)] = 1
        pr, pc = H.positives_from_dense(dev(y))
        b = H.PrefixBatch(po_rel=dev(po[0]), po_obj=dev(po[1]), sp_subj=dev(sp[0]), sp_rel=dev(sp[1]), pos_row=pr, pos_col=pc)
        if n_cand is None:
            b.cand_first, b.n_cand = 2, n_ent - 2
        else:
            b.cand_ids, b.n_cand, b.cand_unique = dev(cand.astype(np.int32)), len(cand), True
        out.append((b, po, sp, cand, y))
    return E, R, out


@pytest.mark.parametrize("d", [16, 520], ids=["dense_d16", "wide_d520"])
def test_l2_reg_zero_is_the_step_without_the_keyword(okge_lib, d):
    """(every row named once per batch: two runs of the SAME step are bit-equal only where its float atomics are order-free)"""
    from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep
    E, R, probs = _problems(3, d, 90, 30, 7, 6, seed=40 + d, once=True, n_cand=50)
    a = FusedTrainStep(dev(E.copy()), dev(R.copy()), "complex", lr=0.3, input_dropout=0.3, seed=5)
    b = FusedTrainStep(dev(E.copy()), dev(R.copy()), "complex", lr=0.3, input_dropout=0.3, seed=5, l2_reg=0.0, l2_reg_dropout=0.2,
                       l2_reg_per_direction=True)
    okge_lib.okge_timing_enable(1)
    okge_lib.okge_timing_reset()
    for p in probs:
        la, lb = a.step(p[0]).clone(), b.step(p[0]).clone()
        assert torch.equal(_bits(la), _bits(lb))
    torch.cuda.synchronize()
    from open_knowledge_graph_embeddings_amd import _native
    timers = _native.timing_collect()
    okge_lib.okge_timing_enable(0)
    assert "n3" not in timers and timers                                   # nothing new is launched
    for name in ("E", "R", "dE", "dR", "sumE", "sumR"):
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    assert float(b.reg_out) == 0.0


@pytest.mark.parametrize("d,per_direction", [(16, False), (520, True)], ids=["dense_d16", "wide_d520_per_direction"])
def test_three_steps_against_float64_and_adagrad(okge_lib, d, per_direction):
    """under the G3 rule of test_wide_shapes / test_hip_parity: each step restarted from the state it is compared with, every
    element within test_oracle_golden.adagrad_tol, 97 % within 2e-6, the accumulators' roots within 1e-4; loss 3e-5, hook 1e-5"""
    from test_oracle_golden import adagrad_tol
    from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep
    n_ent, n_rel, lr, eps, l2, dp = 120, 8, 0.3, 1e-8, 0.05, 0.4
    E, R, probs = _problems(3, d, n_ent, n_rel, 9, 8, seed=50 + d)
    ts = FusedTrainStep(dev(E), dev(R), "complex", lr=lr, l2_reg=l2, l2_reg_dropout=dp, l2_reg_per_direction=per_direction)
    for s, (b, po, sp, cand, y) in enumerate(probs):
        Eo, Ro, sE, sR = (x.cpu().numpy().copy() for x in (ts.E, ts.R, ts.sumE, ts.sumR))
        pE, pR = sE.copy(), sR.copy()
        normalizer = float(y.size)
        ref = ko.step_forward_backward(ko.COMPLEX, Eo.astype(np.float64), Ro.astype(np.float64), po, sp, cand, y.astype(np.float64))
        reg = nr.n3_term(Eo, Ro, po, sp, cand, nr.coef(l2, dp), 2 if per_direction else 1, normalizer)
        assert np.abs(reg["dE"]).max() > 1e-3 * np.abs(ref["dE"]).max()      # the term is no rounding matter here
        loss = float(ts.step(b)[0])
        assert abs(loss - ref["loss"]) <= 3e-5 * abs(ref["loss"])
        assert abs(float(ts.reg_out) - reg["value"]) <= 1e-5 * abs(reg["value"])
        ko.adagrad_step(Eo, (ref["dE"] + reg["dE"]).astype(np.float32), sE, lr)
        ko.adagrad_step(Ro, (ref["dR"] + reg["dR"]).astype(np.float32), sR, lr)
        for mine, ref_, s_mine, s_ref, s_prev in ((ts.E, Eo, ts.sumE, sE, pE), (ts.R, Ro, ts.sumR, sR, pR)):
            tol = adagrad_tol(s_ref, s_prev, lr, eps)
            diff = np.abs(mine.cpu().numpy() - ref_)
            print(f"n3 step {s} d={d}: max diff / tol = {float((diff / tol).max()):.3f}, within 2e-6: {np.mean(diff <= 2e-6):.4f}")
            assert np.all(diff <= tol), float((diff / tol).max())
            assert np.mean(diff <= 2e-6) > 0.97
            np.testing.assert_allclose(np.sqrt(s_mine.cpu().numpy()), np.sqrt(s_ref), rtol=1e-4, atol=1e-6 * np.sqrt(s_ref.max()))


def test_accumulation_and_clipping_take_the_term_per_batch(okge_lib):
    """accumulate = 2 with grad_clip: the clipped sum of two batches' gradients, each with its own l2_reg term, in float64"""
    from test_oracle_golden import adagrad_tol
    from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep
    d, lr, eps, l2, clip = 16, 0.3, 1e-8, 0.05, 0.0004
    E, R, probs = _problems(2, d, 120, 8, 9, 8, seed=77)
    ts = FusedTrainStep(dev(E), dev(R), "distmult", lr=lr, l2_reg=l2, grad_clip=clip, accumulate=2)
    Eo, Ro, sE, sR = E.copy(), R.copy(), np.zeros_like(E), np.zeros_like(R)
    gE, gR = np.zeros(E.shape), np.zeros(R.shape)
    for b, po, sp, cand, y in probs:
        ref = ko.step_forward_backward(ko.DISTMULT, E.astype(np.float64), R.astype(np.float64), po, sp, cand, y.astype(np.float64))
        reg = nr.n3_term(E, R, po, sp, cand, l2, 1, float(y.size))
        gE, gR = gE + ref["dE"] + reg["dE"], gR + ref["dR"] + reg["dR"]
        ts.step(b)
    norm = np.sqrt((gE ** 2).sum() + (gR ** 2).sum())
    assert norm > clip
    scale = min(1.0, clip / (norm + 1e-6))
    ko.adagrad_step(Eo, (gE * scale).astype(np.float32), sE, lr)
    ko.adagrad_step(Ro, (gR * scale).astype(np.float32), sR, lr)
    for mine, ref_, s_ref in ((ts.E, Eo, sE), (ts.R, Ro, sR)):
        diff = np.abs(mine.cpu().numpy() - ref_)
        assert np.all(diff <= adagrad_tol(s_ref, np.zeros_like(s_ref), lr, eps)) and np.mean(diff <= 2e-6) > 0.97


def _run(E, R, batches, graphed=False, **kw):
    from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep, GraphedTrainStep
    st = FusedTrainStep(dev(E.copy()), dev(R.copy()), "complex", lr=0.3, weight_decay=0.0, input_dropout=0.4, relation_input_dropout=0.2,
                        seed=11, l2_reg=0.05, l2_reg_dropout=0.3, **kw)
    gs = GraphedTrainStep(st, batches[0], pos_capacity=max(b.nnz for b in batches) + 3) if graphed else None
    losses, regs = [], []
    for b in batches:
        losses.append((gs.step(b) if graphed else st.step(b)).clone())
        regs.append(st.reg_out.clone())
    torch.cuda.synchronize()
    return st, losses, regs


def _assert_same(a, b):
    for name in ("E", "R", "sumE", "sumR"):
        assert torch.equal(_bits(getattr(a[0], name)), _bits(getattr(b[0], name))), name
    for xs, ys in zip(a[1:], b[1:]):
        for x, y in zip(xs, ys):
            assert torch.equal(_bits(x), _bits(y))


def test_row_sparse_step_equals_the_dense_step_bit_for_bit(okge_lib):
    """weight_decay = 0, every row named once per batch (see _problems): the dense step adds the term's one addend to the one the
    step left in that row, the row-sparse step adds the same two in its occurrence row -- the same sum"""
    E, R, probs = _problems(3, 200, 400, 30, 6, 5, seed=60, once=True, n_cand=130)
    batches = [p[0] for p in probs]
    dense = _run(E, R, batches)
    sparse = _run(E, R, batches, sparse=True)
    assert sparse[0].dE is None and float(dense[2][0]) > 0
    _assert_same(dense, sparse)
    plain = _run(E, R, batches[:1], l2_reg_per_direction=True)               # (the term moves the tables: not a no-op)
    assert not torch.equal(plain[0].E, _run(E, R, batches[:1])[0].E)


@pytest.mark.parametrize("kw", [dict(), dict(sparse=True)], ids=["dense", "row_sparse"])
def test_graphed_replay_equals_the_eager_step_bit_for_bit(okge_lib, kw):
    E, R, probs = _problems(3, 16, 200, 30, 6, 5, seed=61, once=True, n_cand=70)
    batches = [p[0] for p in probs]
    _assert_same(_run(E, R, batches, **kw), _run(E, R, batches, graphed=True, **kw))


@pytest.mark.parametrize("fast", [False, True], ids=["general", "fast_call"])
def test_fused_route_with_sparse_gradients(okge_lib, fast):
    """AddLossModule(sparse_grads=True, fused_l2_reg=True): the term is added to the occurrence rows; densified, the gradients
    meet the same bounds"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule
    f = nr.fixture_problem(golden("g23_n3_distmult_repeat"))
    m = _model(f)
    mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0, sparse_grads=True, fused_l2_reg=True)
    inputs = [(dev(p[0].astype(np.int32)), dev(p[1].astype(np.int32))) for p in (f["po"], f["sp"])]
    labels = H.positives_from_dense(dev(f["labels"])) if fast else dev(f["labels"])
    loss, hook, _ = mod(inputs=inputs, labels=labels, use_batch_shared_entities=True, batch_shared_entities=dev(f["cand"].astype(np.int32)),
                        epoch=1, input_style_triple_or_prefix="right_and_left_prefix")
    assert abs(float(loss.detach()) - f["loss"]) <= 3e-5 * abs(f["loss"]) and abs(float(hook.detach()) - f["hook"]) <= 1e-5 * abs(f["hook"])
    ((loss.sum() + hook) / f["normalizer"]).backward()
    for p, ref, k in ((m.entity_embedding.weight, f["dE"], "dE"), (m.relation_embedding.weight, f["dR"], "dR")):
        assert p.grad.is_sparse
        np.testing.assert_allclose(p.grad.to_dense().cpu().numpy(), ref, rtol=0, atol=5e-5 * np.abs(ref).max() + 1e-10, err_msg=k)
