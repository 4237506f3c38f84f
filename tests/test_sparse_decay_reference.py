"""CPU checks of the row-sparse step with deferred weight decay: the NumPy statement (tests/sparse_decay_reference.py) against
eager dense `adagrad_step` calls of the oracle at the same weight decay, the Python layer's constructor surface and host-side
bookkeeping, and the two new exports."""
import numpy as np
import pytest
import torch

from oracle import kge_oracle as ko
import sparse_decay_reference as sdr
import sparse_reference as sr

STEPS, D = 20, 8
HP = (0.3, 1e-10, 1e-8)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _id_lists(rng, rows):
    """20 lists with repeats; the last five rows are named by no step, and row 0 by every step"""
    out = []
    for _ in range(STEPS):
        ids = rng.integers(0, rows - 5, rng.integers(3, 9))
        out.append(np.concatenate([[0], ids, ids[:2]]).astype(np.int64))
    return out


@pytest.mark.parametrize("rows", [37, 64])
@pytest.mark.parametrize("window", [1, 2, 3, 8])
def test_deferred_statement_equals_eager_dense_steps(rows, window):
    rng = np.random.default_rng(rows * 10 + window)
    p0 = (rng.standard_normal((rows, D)) * 0.1).astype(np.float32)
    lists = _id_lists(rng, rows)
    grads = [(rng.standard_normal((len(ids), D)) * 1e-2).astype(np.float32) for ids in lists]
    assert any(len(np.unique(ids)) < len(ids) for ids in lists)
    never = np.setdiff1d(np.arange(rows), np.concatenate(lists))
    assert never.size >= 5

    eager_p, eager_s = p0.copy(), np.zeros_like(p0)
    lazy = sdr.DeferredTable(p0.copy(), np.zeros_like(p0), *HP)
    lagged = False
    for ids, g in zip(lists, grads):
        lazy.catch_up(ids)
        named = np.unique(ids)
        # what the forward reads: every named row holds its eager value
        assert np.array_equal(_bits(lazy.p[named]), _bits(eager_p[named])) and np.array_equal(_bits(lazy.s[named]), _bits(eager_s[named]))
        assert (lazy.row_steps[named] == lazy.T).all()
        lagged = lagged or bool((lazy.row_steps < lazy.T).any())
        lazy.update(ids, g)
        lazy.due_slice(window)
        dense, _ = sr.coalesce(ids, g, rows)
        ko.adagrad_step(eager_p, dense, eager_s, *HP)
        assert lazy.row_steps.max() == lazy.T and lazy.row_steps.min() >= lazy.T - (window - 1)
    assert lagged == (window > 1)                       # W > 1: some row lagged at some point, or the test shows nothing
    lazy.flush()
    assert lazy.T == STEPS and (lazy.row_steps == STEPS).all()
    assert np.array_equal(_bits(lazy.p), _bits(eager_p)) and np.array_equal(_bits(lazy.s), _bits(eager_s))
    assert not np.array_equal(lazy.p[never], p0[never])     # the decay is real: a row no step named has moved


def test_update_without_catch_up_replays_the_lagging_rows():
    rng = np.random.default_rng(7)
    p0 = (rng.standard_normal((37, D)) * 0.1).astype(np.float32)
    eager_p, eager_s = p0.copy(), np.zeros_like(p0)
    lazy = sdr.DeferredTable(p0.copy(), np.zeros_like(p0), *HP)
    for t in range(9):
        ids = np.array([t % 5, 30, 30, (3 * t) % 29])
        g = (rng.standard_normal((4, D)) * 1e-2).astype(np.float32)
        if t == 8:
            assert lazy.row_steps[ids].min() < lazy.T    # a named row lags and nobody caught it up
        lazy.update(ids, g)
        lazy.due_slice(8)
        dense, _ = sr.coalesce(ids, g, 37)
        ko.adagrad_step(eager_p, dense, eager_s, *HP)
    lazy.flush()
    assert np.array_equal(_bits(lazy.p), _bits(eager_p)) and np.array_equal(_bits(lazy.s), _bits(eager_s))


# ---- the Python layer (no GPU: refusals are raised, and buffers made, before anything touches a device) ------------------------
def test_fused_train_step_decay_window_surface():
    from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep
    E, R = torch.zeros(6, 8), torch.zeros(3, 8)
    st = FusedTrainStep(E, R, "complex", sparse=True, weight_decay=1e-10, decay_window=4, engine=object())
    assert st.decay_window == 4 and st.dE is None and st._pending is None
    assert st.rowsE.dtype == torch.int32 and st.rowsE.shape == (6,) and st.rowsR.shape == (3,) and st._counters.tolist() == [0, 0]
    with pytest.raises(NotImplementedError, match="multiple of 4"):
        FusedTrainStep(torch.zeros(6, 6), torch.zeros(3, 6), "complex", sparse=True, weight_decay=1e-10, decay_window=4, engine=object())
    with pytest.raises(NotImplementedError, match="grad_clip"):
        FusedTrainStep(E, R, "complex", sparse=True, weight_decay=1e-10, decay_window=4, grad_clip=1.0, engine=object())
    with pytest.raises(NotImplementedError, match="accumulate"):
        FusedTrainStep(E, R, "complex", sparse=True, weight_decay=1e-10, decay_window=4, accumulate=2, engine=object())
    with pytest.raises(ValueError, match="decay_window"):
        FusedTrainStep(E, R, "complex", weight_decay=1e-10, decay_window=4, engine=object())         # the dense step has no deferral
    with pytest.raises(ValueError, match="decay_window"):
        FusedTrainStep(E, R, "complex", sparse=True, weight_decay=1e-10, decay_window=0, engine=object())
    with pytest.raises(ValueError, match="weight_decay option is not compatible with sparse gradients"):
        FusedTrainStep(E, R, "complex", sparse=True, weight_decay=1e-10, engine=object())            # decay_window=None: as before


def test_deferred_step_bookkeeping_on_the_host():
    """a recording stand-in for the engine: an optimizer step leaves work pending under the hyper-parameters of ITS time, flush()
    settles it once with exactly those, a learning-rate change settles before the next launch, a graph replay marks work pending
    again, state_tensors() flushes and carries the step counters, and the checkpoint writer flushes"""
    from open_knowledge_graph_embeddings_amd.checkpoint import to_reference_checkpoint
    from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep

    class Engine:
        def __init__(self):
            self.calls = []

        def adagrad_rows_decay(self, tensors, counters, window, lr, wd, eps):
            self.calls.append(("step", len(tensors), window, lr, wd, eps))

        def adagrad_lazy(self, tensors, counters, window, flush, lr, wd, eps):
            assert flush and all(t[1] is t[2] for t in tensors)        # the accumulator stands in for the gradient
            self.calls.append(("flush", len(tensors), window, lr, wd, eps))

    def make(window):
        eng = Engine()
        st = FusedTrainStep(torch.zeros(6, 8), torch.zeros(3, 8), "complex", lr=0.1, sparse=True, weight_decay=1e-10, decay_window=window,
                            engine=eng)
        st._cur_rows = dict(idE=None, gE=None, idR=None, gR=None)
        return st, eng
    st, eng = make(8)
    st.flush()
    assert eng.calls == []                                          # nothing owed, nothing launched
    st.optimizer_step()
    assert eng.calls == [("step", 2, 8, 0.1, 1e-10, 1e-8)] and st._pending == (0.1, 1e-10, 1e-8)
    st.lr = 0.05                                                     # the owed steps keep the rate of their time
    st.optimizer_step()
    assert eng.calls[1] == ("flush", 2, 8, 0.1, 1e-10, 1e-8) and eng.calls[2] == ("step", 2, 8, 0.05, 1e-10, 1e-8)
    st.flush()
    st.flush()
    assert [c[0] for c in eng.calls] == ["step", "flush", "step", "flush"] and st._pending is None
    st.mark_pending()                                                # GraphedTrainStep.replay: the graph ran the step's launches
    tensors = st.state_tensors()
    assert eng.calls[-1][0] == "flush" and len(eng.calls) == 5
    assert [t.data_ptr() for t in tensors] == [t.data_ptr() for t in (st.E, st.R, st.sumE, st.sumR, st.rowsE, st.rowsR, st._counters)]
    st.mark_pending()
    to_reference_checkpoint(st)
    assert eng.calls[-1][0] == "flush" and len(eng.calls) == 6 and st._pending is None
    from open_knowledge_graph_embeddings_amd.checkpoint import load_reference_checkpoint
    ckpt = to_reference_checkpoint(st)
    ckpt["state_dict"] = {k: v + 1 for k, v in ckpt["state_dict"].items()}
    st.mark_pending()
    load_reference_checkpoint(st, ckpt)                              # owed steps are settled BEFORE the tables are overwritten
    assert eng.calls[-1][0] == "flush" and len(eng.calls) == 7 and st._pending is None and bool((st.E == 1).all())
    st, eng = make(1)                                                # window 1: every row every step, nothing is ever owed
    st.optimizer_step()
    assert st._pending is None


def test_library_exports_the_deferred_decay_entry_points():
    from open_knowledge_graph_embeddings_amd import _native
    if _native.needs_build():
        _native.build_native()
    L = _native.lib()
    assert {"okge_rows_catch_up", "okge_adagrad_rows_decay"} <= set(_native.EXPORTS)
    assert L.okge_rows_catch_up is not None and L.okge_adagrad_rows_decay is not None
    # argument errors are answered before anything touches a device
    t = _native.RowsDecayTensor()
    assert L.okge_rows_catch_up(t, 1, None, 0.3, 1e-10, 1e-8, None) == -1
    assert L.okge_adagrad_rows_decay(t, 1, None, 4, 0.3, 1e-10, 1e-8, None, 0, None) == -1
