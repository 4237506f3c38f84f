"""FusedTrainStep(sparse=True, weight_decay=1e-10, decay_window=4): the row-sparse step with the reference's weight decay, its
decay-only updates deferred, against the dense FusedTrainStep at the same weight decay.

The batches are tests/test_sparse_step.py's light ones (400 entities, 14 relations, 130 candidates, n_po 5, n_sp 6): every entity
and relation row receives at most two contributions (asserted), so the dense step's float atomics are order-free and the two
steps can be compared bit for bit.  A bit-equal loss at EVERY step shows that the rows a batch names were caught up before the
forward read them; bit-equal tables and accumulators after flush() show the rest."""
import numpy as np
import pytest
import torch

from open_knowledge_graph_embeddings_amd.checkpoint import to_reference_checkpoint
from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep, GraphedTrainStep
from test_sparse_step import N_CAND, N_ENT, _batch, _bits, _tables

STEPS, WINDOW, WD = 14, 4, 1e-10


def _batches(seed):
    rng = np.random.default_rng(seed)
    made = [_batch(rng) for _ in range(STEPS)]
    for _, ids_e, ids_r in made:                      # what makes the dense step's atomics order-free
        assert np.bincount(ids_e).max() == 2 and np.bincount(ids_r).max() == 2
        assert len(np.unique(ids_e[:N_CAND])) == N_CAND
    return [m[0] for m in made], np.unique(np.concatenate([m[1] for m in made]))


def _steps(scorer, d, dropout, batches, deferred, graphed=False, lr_after_5=None):
    E, R = _tables(3, d)
    kw = dict(sparse=True, decay_window=WINDOW) if deferred else {}
    st = FusedTrainStep(E, R, scorer, lr=0.3, weight_decay=WD, eps=1e-8, input_dropout=dropout, relation_input_dropout=dropout / 2,
                        seed=11, label_smoothing=0.1, **kw)
    losses = []
    gs = GraphedTrainStep(st, batches[0], pos_capacity=max(b.nnz for b in batches)) if graphed else None
    for i, b in enumerate(batches):
        if i == 5 and lr_after_5 is not None:
            st.lr = lr_after_5
        losses.append((gs.step(b) if graphed else st.step(b)).clone())
    torch.cuda.synchronize()
    return st, losses


def _assert_same(a, b, losses_a, losses_b):
    for x, y in zip(losses_a, losses_b):
        assert torch.equal(_bits(x), _bits(y))
    for name in ("E", "R", "sumE", "sumR"):
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name


@pytest.mark.gpu
@pytest.mark.parametrize("scorer,d,dropout", [("complex", 200, 0.4), ("distmult", 264, 0.25)])
def test_deferred_step_equals_dense_step_at_the_reference_weight_decay(okge_lib, scorer, d, dropout):
    batches, named = _batches(d)
    dense, dense_losses = _steps(scorer, d, dropout, batches, deferred=False)
    lazy, lazy_losses = _steps(scorer, d, dropout, batches, deferred=True)
    assert lazy.dE is None and lazy.dR is None
    for x, y in zip(dense_losses, lazy_losses):        # every step: the catch-up precedes the forward
        assert torch.equal(_bits(x), _bits(y))
    T = int(lazy._counters[0].item())
    assert T == STEPS and int(lazy._counters[1].item()) == 0
    assert bool((lazy.rowsE < T).any()) and int(lazy.rowsE.min().item()) >= T - (WINDOW - 1)      # the deferral happened
    assert not torch.equal(_bits(lazy.E), _bits(dense.E))                                       # ... and shows before the flush
    lazy.flush()
    assert bool((lazy.rowsE == T).all()) and bool((lazy.rowsR == T).all())
    _assert_same(dense, lazy, dense_losses, lazy_losses)
    E0, _ = _tables(3, d)
    unnamed = torch.from_numpy(np.setdiff1d(np.arange(N_ENT), named)).cuda()
    assert unnamed.numel() >= 2                        # (entities 0 and 1 at least: no batch names them)
    moved = (_bits(lazy.E[unnamed]) != _bits(E0[unnamed])).any(dim=1)
    assert bool(moved.all())                           # the decay is real: rows no batch named have moved
    snap = [t.clone() for t in (lazy.E, lazy.R, lazy.sumE, lazy.sumR, lazy.rowsE, lazy.rowsR, lazy._counters)]
    lazy.flush()                                       # a second flush: nothing owed, nothing moves
    lazy.mark_pending()
    lazy.flush()                                       # ... and one that does launch finds every row current
    for t, s0 in zip((lazy.E, lazy.R, lazy.sumE, lazy.sumR, lazy.rowsE, lazy.rowsR, lazy._counters), snap):
        assert torch.equal(t, s0)


@pytest.mark.gpu
def test_graphed_deferred_step_replays_equal_eager_steps(okge_lib):
    batches, _ = _batches(2)
    eager, le = _steps("complex", 200, 0.4, batches, deferred=True)
    graphed, lg = _steps("complex", 200, 0.4, batches, deferred=True, graphed=True)
    assert graphed._pending is not None                # a replay leaves rows owing steps again
    assert torch.equal(eager.rowsE, graphed.rowsE) and torch.equal(eager._counters, graphed._counters)
    eager.flush()
    graphed.flush()
    _assert_same(eager, graphed, le, lg)
    dense, ld = _steps("complex", 200, 0.4, batches, deferred=False)
    _assert_same(dense, graphed, ld, lg)


@pytest.mark.gpu
def test_learning_rate_change_settles_pending_steps_first(okge_lib):
    batches, _ = _batches(5)
    dense, ld = _steps("complex", 200, 0.4, batches, deferred=False, lr_after_5=0.1)
    lazy, ll = _steps("complex", 200, 0.4, batches, deferred=True, lr_after_5=0.1)
    lazy.flush()
    _assert_same(dense, lazy, ld, ll)
    plain, lp = _steps("complex", 200, 0.4, batches, deferred=False)
    assert not torch.equal(_bits(plain.E), _bits(dense.E))        # (the change of rate is visible at all)


@pytest.mark.gpu
def test_checkpoint_of_the_deferred_step_is_the_dense_step_s(okge_lib):
    batches, _ = _batches(8)
    dense, _ = _steps("distmult", 264, 0.25, batches, deferred=False)
    lazy, _ = _steps("distmult", 264, 0.25, batches, deferred=True)
    assert lazy._pending is not None
    a, b = to_reference_checkpoint(dense), to_reference_checkpoint(lazy)      # (flushes the deferred step)
    assert lazy._pending is None
    assert a["training_steps"] == b["training_steps"] == STEPS
    for key in a["state_dict"]:
        assert torch.equal(_bits(a["state_dict"][key]), _bits(b["state_dict"][key])), key
    sa, sb = (c["optimizer_state_dict"][0]["optimizer_state"]["state"] for c in (a, b))
    for k in (0, 1):
        assert torch.equal(_bits(sa[k]["sum"]), _bits(sb[k]["sum"])) and torch.equal(sa[k]["step"], sb[k]["step"])
    assert a["optimizer_state_dict"][0]["optimizer_state"]["param_groups"] == b["optimizer_state_dict"][0]["optimizer_state"]["param_groups"]
