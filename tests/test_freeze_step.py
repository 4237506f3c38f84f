"""FusedTrainStep(freeze="entities" | "relations"): the reference's resume_freeze (trainer.py:532-536) on the fused step.

Batches are order-free (test_n3_step._problems(once=True): unique sampled candidates, every prefix id once, no prefix entity a
candidate), so "equal" below is bit-equal.  Against float64 the G3 rule of test_hip_parity.test_g3_adagrad_steps holds: each step
is compared from the state it started in -- the loss within 2e-5 relative, the trained table's gradient within 2e-5 of its
largest element (the bound smoke() holds the step to), the Adagrad update from the oracle's gradient within
test_oracle_golden.adagrad_tol with 97 % of the elements within 2e-6, the Adam update from the gradient the device left within
adam_reference's caps (test_adam_step._hold) -- with the frozen table held fixed in the oracle."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_reference as A  # noqa: E402
import wide_reference as wr  # noqa: E402
from oracle import kge_oracle as ko  # noqa: E402
from test_adam_step import _hold  # noqa: E402
from test_n3_step import _problems, dev  # noqa: E402
from test_oracle_golden import adagrad_tol  # noqa: E402

pytestmark = pytest.mark.gpu
LR = {"adagrad": 0.3, "adam": 1e-2}
WD, EPS, P_DROP, SEED = 1e-10, 1e-8, 0.4, 77


def _step(E, R, scorer, **kw):
    from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep
    opt = kw.get("optimizer", "adagrad")
    kw.setdefault("lr", LR[opt])
    kw.setdefault("weight_decay", WD)
    return FusedTrainStep(dev(E.copy()), dev(R.copy()), scorer, eps=EPS, seed=SEED, **kw)


def _np(t):
    return t.detach().cpu().numpy().copy()


def _trained(ts):
    """(table, gradient, state tensors) of the table a frozen step trains"""
    e = ts.freeze == "relations"
    if ts.optimizer == "adam":
        return (ts.E, ts.dE, (ts.mE, ts.vE)) if e else (ts.R, ts.dR, (ts.mR, ts.vR))
    return (ts.E, ts.dE, (ts.sumE,)) if e else (ts.R, ts.dR, (ts.sumR,))


def _frozen_parts(ts):
    """the frozen table and every attribute that could hold a gradient or state of it"""
    tag = "E" if ts.freeze == "entities" else "R"
    return getattr(ts, tag), [getattr(ts, n + tag, None) for n in ("d", "sum", "m", "v", "adam_state")]


def _oracle(scorer, E, R, prob, step_no, p_ent, normalizer=None):
    """the float64 step on fp32 tables with the masks FusedTrainStep draws at its step `step_no`"""
    _, po, sp, cand, y = prob
    masks = wr.philox_masks(SEED, step_no, len(po[0]), len(sp[0]), len(cand), E.shape[1], p_ent, 0.0) if p_ent > 0 else {}
    return ko.step_forward_backward(ko.KIND_NAMES[scorer], E.astype(np.float64), R.astype(np.float64), po, sp, cand, y.astype(np.float64),
                                    normalizer=normalizer, p_ent=p_ent, **{k: v for k, v in masks.items() if v is not None})


class GradSpy:
    """the trained table's gradient as the optimizer sweep finds it (the sweep clears it)"""

    def __init__(self, ts):
        self.grads = []
        inner = ts.optimizer_step

        def wrapped(lazy_zero=False):
            torch.cuda.synchronize()
            self.grads.append(_np(_trained(ts)[1]))
            inner(lazy_zero=lazy_zero)
        ts.optimizer_step = wrapped


@pytest.mark.parametrize("freeze", ["entities", "relations"])
@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
@pytest.mark.parametrize("scorer,d", [("complex", 24), ("distmult", 300)])
def test_three_steps(okge_lib, scorer, d, optimizer, freeze):
    E, R, probs = _problems(3, d, 420, 90, 33, 32, seed=d, once=True, n_cand=200)
    ts = _step(E, R, scorer, optimizer=optimizer, input_dropout=P_DROP, freeze=freeze)
    plain = _step(E, R, scorer, optimizer=optimizer, input_dropout=P_DROP)
    table0, others = _frozen_parts(ts)
    assert all(x is None for x in others)                      # no gradient, no state: not even allocated
    frozen0 = table0.clone()
    spy = GradSpy(ts)
    key = "dE" if freeze == "relations" else "dR"
    lr = LR[optimizer]
    for i, prob in enumerate(probs):
        table, _, state = _trained(ts)
        p0, s0 = _np(table), [_np(s) for s in state]
        ref = _oracle(scorer, _np(ts.E), _np(ts.R), prob, i + 1, P_DROP)
        loss = float(ts.step(prob[0])[0])
        torch.cuda.synchronize()
        assert abs(loss - ref["loss"]) <= 2e-5 * abs(ref["loss"]), (i, loss, ref["loss"])
        g = spy.grads[i]
        gmax = np.abs(ref[key]).max()
        print(f"freeze-step {scorer}-d{d}-{optimizer}-{freeze} step {i}: loss_rel={abs(loss - ref['loss']) / abs(ref['loss']):.2e} "
              f"grad_err/max={np.abs(g - ref[key]).max() / gmax:.2e}")
        np.testing.assert_allclose(g, ref[key], rtol=0, atol=2e-5 * gmax)
        p1, s1 = _np(table), [_np(s) for s in state]
        if optimizer == "adagrad":
            want_p, want_s = p0.copy(), s0[0].copy()
            ko.adagrad_step(want_p, ref[key].astype(np.float32), want_s, lr, WD, EPS)
            tol = adagrad_tol(want_s, s0[0], lr, EPS)
            diff = np.abs(p1 - want_p)
            print(f"    adagrad: max diff / tol = {float((diff / tol).max()):.3f}, within 2e-6: {np.mean(diff <= 2e-6):.4f}")
            assert np.all(diff <= tol), float((diff / tol).max())
            assert np.mean(diff <= 2e-6) > 0.97
            np.testing.assert_allclose(np.sqrt(s1[0]), np.sqrt(want_s), rtol=1e-4, atol=1e-6 * np.sqrt(want_s.max()))
        else:
            assert ts.adam_t == i + 1
            r = A.adam64(p0, g, s0[0], s0[1], i + 1, lr, ts.betas, EPS, WD)
            _hold(f"{scorer}-d{d}-{freeze} step{i}", [p1, s1[0], s1[1]], r, s0[0], s0[1])
        if i == 0:                                             # the unfrozen step from the same state: the trained table's bits
            plain.step(prob[0])
            torch.cuda.synchronize()
            assert torch.equal(table, plain.E if freeze == "relations" else plain.R)
            assert not torch.equal(table0, plain.E if freeze == "entities" else plain.R)       # (which does move the other table)
    assert torch.equal(table0, frozen0)
    assert all(x is None for x in _frozen_parts(ts)[1])


@pytest.mark.parametrize("freeze", ["entities", "relations"])
def test_one_vs_all_steps(okge_lib, freeze):
    """1-vs-all with repeated prefix ids, three steps: the entity gradient a step leaves for the next one to overwrite (the
    lazy zero_grad of the 1-vs-all step) must not leak into it.  Each Adagrad step against the oracle's from the same state"""
    E, R, probs = _problems(3, 24, 150, 12, 9, 8, seed=31)
    ts = _step(E, R, "complex", freeze=freeze, input_dropout=P_DROP)
    frozen0 = _frozen_parts(ts)[0].clone()
    key = "dE" if freeze == "relations" else "dR"
    for i, prob in enumerate(probs):
        table, _, (s,) = _trained(ts)
        p0, s0 = _np(table), _np(s)
        ref = _oracle("complex", _np(ts.E), _np(ts.R), prob, i + 1, P_DROP)
        loss = float(ts.step(prob[0])[0])
        torch.cuda.synchronize()
        assert abs(loss - ref["loss"]) <= 2e-5 * abs(ref["loss"])
        want_p, want_s = p0.copy(), s0.copy()
        ko.adagrad_step(want_p, ref[key].astype(np.float32), want_s, LR["adagrad"], WD, EPS)
        diff = np.abs(_np(table) - want_p)
        assert np.all(diff <= adagrad_tol(want_s, s0, LR["adagrad"], EPS)), (i, float(diff.max()))
        assert np.mean(diff <= 2e-6) > 0.97
        np.testing.assert_allclose(np.sqrt(_np(s)), np.sqrt(want_s), rtol=1e-4, atol=1e-6 * np.sqrt(want_s.max()))
    assert torch.equal(_frozen_parts(ts)[0], frozen0)


def test_zero_gradient_is_not_a_freeze(okge_lib):
    """why the flag exists ("The untouched slot"): Adagrad on an all-zero gradient still moves a 0.3-sized weight by
    ~3e-4 on the first step (weight_decay 1e-10 against eps 1e-8)"""
    from open_knowledge_graph_embeddings_amd.hotpath import HotPath
    hp = HotPath("cuda:0")
    p, g, s = torch.full((4, 8), 0.3, device="cuda:0"), torch.zeros((4, 8), device="cuda:0"), torch.zeros((4, 8), device="cuda:0")
    hp.adagrad(p, g, s, 0.3, 1e-10, 1e-8)
    assert 1e-4 < float((p - 0.3).abs().max()) < 1e-3


@pytest.mark.parametrize("freeze", ["entities", "relations"])
def test_grad_clip_sees_the_trained_gradient_alone(okge_lib, freeze):
    """normalizer = 1 makes grad_clip = 0.5 bind; grad_norm is the norm of the trained table's raw gradient, the update is
    Adagrad's on that gradient times the coefficient of clip_grad_norm_ (max_norm / (norm + 1e-6))"""
    E, R, probs = _problems(1, 24, 300, 80, 20, 17, seed=5, once=True, n_cand=150)
    raw = _step(E, R, "complex", freeze=freeze)
    raw.steps = 1
    raw.forward_backward(probs[0][0], normalizer=1.0)
    torch.cuda.synchronize()
    g = _np(_trained(raw)[1]).astype(np.float64)
    norm = np.sqrt((g ** 2).sum())
    assert norm > 0.5
    ts = _step(E, R, "complex", freeze=freeze, grad_clip=0.5)
    frozen0 = _frozen_parts(ts)[0].clone()
    ts.step(probs[0][0], normalizer=1.0)
    torch.cuda.synchronize()
    assert abs(float(ts.grad_norm[0]) - norm) <= 1e-6 * norm, (float(ts.grad_norm[0]), norm)
    table, _, (s,) = _trained(ts)
    p0 = E if freeze == "relations" else R
    want_p, want_s = p0.copy(), np.zeros_like(p0)
    ko.adagrad_step(want_p, (g * (0.5 / (norm + 1e-6))).astype(np.float32), want_s, LR["adagrad"], WD, EPS)
    diff = np.abs(_np(table) - want_p)
    assert np.all(diff <= adagrad_tol(want_s, np.zeros_like(want_s), LR["adagrad"], EPS))
    np.testing.assert_allclose(np.sqrt(_np(s)), np.sqrt(want_s), rtol=1e-4, atol=1e-6 * np.sqrt(want_s.max()))
    assert torch.equal(_frozen_parts(ts)[0], frozen0)


@pytest.mark.parametrize("freeze", ["entities", "relations"])
def test_accumulate(okge_lib, freeze):
    """accumulate = 2: no update after the first batch; after the second the trained table is the unfrozen accumulate = 2
    step's bit for bit, and Adagrad's on the sum of the two float64 gradients"""
    E, R, probs = _problems(2, 24, 300, 80, 20, 17, seed=6, once=True, n_cand=150)
    ts, plain = _step(E, R, "complex", freeze=freeze, accumulate=2), _step(E, R, "complex", accumulate=2)
    ts.step(probs[0][0])
    plain.step(probs[0][0])
    torch.cuda.synchronize()
    assert torch.equal(ts.E, dev(E)) and torch.equal(ts.R, dev(R))
    ts.step(probs[1][0])
    plain.step(probs[1][0])
    torch.cuda.synchronize()
    key = "dE" if freeze == "relations" else "dR"
    table, grad, (s,) = _trained(ts)
    assert torch.equal(table, plain.E if freeze == "relations" else plain.R) and not bool(grad.any())
    assert torch.equal(_frozen_parts(ts)[0], dev(E if freeze == "entities" else R))
    g = sum(_oracle("complex", E, R, p, 0, 0.0)[key] for p in probs)
    p0 = E if freeze == "relations" else R
    want_p, want_s = p0.copy(), np.zeros_like(p0)
    ko.adagrad_step(want_p, g.astype(np.float32), want_s, LR["adagrad"], WD, EPS)
    assert np.all(np.abs(_np(table) - want_p) <= adagrad_tol(want_s, np.zeros_like(want_s), LR["adagrad"], EPS))


@pytest.mark.parametrize("freeze", ["entities", "relations"])
def test_wide_step(okge_lib, freeze):
    """d = 1024, one step with dropout: the trained table is the unfrozen step's, the frozen one keeps its bits"""
    E, R, probs = _problems(1, 1024, 260, 60, 20, 17, seed=8, once=True, n_cand=150)
    ts, plain = _step(E, R, "distmult", freeze=freeze, input_dropout=P_DROP), _step(E, R, "distmult", input_dropout=P_DROP)
    ref = _oracle("distmult", E, R, probs[0], 1, P_DROP)
    la, lb = float(ts.step(probs[0][0])[0]), float(plain.step(probs[0][0])[0])
    torch.cuda.synchronize()
    assert la == lb and abs(la - ref["loss"]) <= 3e-5 * abs(ref["loss"])
    assert torch.equal(_trained(ts)[0], plain.E if freeze == "relations" else plain.R)
    assert torch.equal(_frozen_parts(ts)[0], dev(E if freeze == "entities" else R))


@pytest.mark.parametrize("freeze,optimizer", [("entities", "adagrad"), ("relations", "adam")])
def test_graphed_step_equals_the_eager_step(okge_lib, freeze, optimizer):
    """five replays under GraphedTrainStep against the eager step, d = 300 (the stream-K tile launch), input dropout 0.4"""
    from open_knowledge_graph_embeddings_amd.train_step import GraphedTrainStep
    E, R, probs = _problems(3, 300, 420, 90, 33, 32, seed=11, once=True, n_cand=200)
    eager = _step(E, R, "distmult", freeze=freeze, optimizer=optimizer, input_dropout=P_DROP)
    inner = _step(E, R, "distmult", freeze=freeze, optimizer=optimizer, input_dropout=P_DROP)
    graphed = GraphedTrainStep(inner, probs[0][0], pos_capacity=max(p[0].nnz for p in probs) + 5)
    assert torch.equal(inner.E, dev(E)) and torch.equal(inner.R, dev(R))       # the warm-up steps did not count
    for i in range(5):
        le, lg = float(eager.step(probs[i % 3][0])[0]), float(graphed.step(probs[i % 3][0])[0])
        assert le == lg, (i, le, lg)
    torch.cuda.synchronize()
    assert torch.equal(inner.E, eager.E) and torch.equal(inner.R, eager.R)
    for a, b in zip(_trained(inner)[2], _trained(eager)[2]):
        assert torch.equal(a, b)
    assert torch.equal(_frozen_parts(inner)[0], dev(E if freeze == "entities" else R))
    assert not torch.equal(_trained(inner)[0], dev(R if freeze == "entities" else E))


@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
def test_checkpoint_resume_is_bit_identical(okge_lib, tmp_path, optimizer):
    """saved after step 2, loaded into a fresh frozen step and, through freeze_param, into a step built unfrozen: step 3 is the
    uninterrupted run's.  The file holds the frozen table and, for Adagrad, its untouched `sum`; for Adam no entry"""
    from open_knowledge_graph_embeddings_amd import checkpoint as C
    E, R, probs = _problems(3, 24, 300, 80, 20, 17, seed=12, once=True, n_cand=150)
    kw = dict(optimizer=optimizer, input_dropout=P_DROP)
    run = _step(E, R, "complex", freeze="entities", **kw)
    for p in probs[:2]:
        run.step(p[0])
    path = str(tmp_path / "frozen.pt")
    C.save_checkpoint(path, run)
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    state = ckpt["optimizer_state_dict"][0]["optimizer_state"]["state"]
    assert torch.equal(ckpt["state_dict"][C.ENTITY_KEY], torch.from_numpy(E))
    if optimizer == "adagrad":
        assert not bool(state[0]["sum"].any()) and float(state[0]["step"]) == 0 and float(state[1]["step"]) == 2
    else:
        assert 0 not in state and float(state[1]["step"]) == 2
    fresh = _step(np.zeros_like(E), np.zeros_like(R), "complex", freeze="entities", **kw)
    C.load_reference_checkpoint(fresh, path)
    named = _step(np.zeros_like(E), np.zeros_like(R), "complex", **kw)
    C.load_reference_checkpoint(named, path, freeze_param=[C.ENTITY_KEY])
    assert named.freeze == "entities" and named.dE is None
    losses = [float(s.step(probs[2][0])[0]) for s in (run, fresh, named)]
    torch.cuda.synchronize()
    assert losses[0] == losses[1] == losses[2]
    for other in (fresh, named):
        assert other.steps == run.steps == 3
        assert torch.equal(other.R, run.R) and torch.equal(other.E, run.E) and torch.equal(other.E, dev(E))
        for a, b in zip(_trained(other)[2], _trained(run)[2]):
            assert torch.equal(a, b)
    if optimizer == "adagrad":                                 # the `sum` that came with the file is carried, untouched
        assert named.sumE is not None and not bool(named.sumE.any())
    with pytest.raises(ValueError, match="nothing is left to train"):
        C.load_reference_checkpoint(_step(E, R, "complex", **kw), path, freeze_param=["True"])
    # resumed UNFROZEN: the step count (it keys the dropout masks) is the run's, not the 0 of the table that never had a gradient
    if optimizer == "adagrad":
        thawed = _step(np.zeros_like(E), np.zeros_like(R), "complex", **kw)
        C.load_reference_checkpoint(thawed, path)
        assert thawed.freeze is None and thawed.steps == 2
        assert not bool(thawed.sumE.any())
