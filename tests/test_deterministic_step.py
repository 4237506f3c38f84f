"""FusedTrainStep(deterministic=True): dense gradients with the order of every row's additions fixed (okge_rows_to_dense).

Small tables on purpose -- 40 entities, 3 relations, prefix entities drawn from 5 ids -- so that every relation row and the five
prefix entities take DOZENS of contributions per batch: the regime in which the default dense step's float atomics make its sums
depend on arrival order and in which it differs from the row-sparse step.  The equalities below hold on such batches only with
the feature."""
import numpy as np
import pytest
import torch

from open_knowledge_graph_embeddings_amd import _native as N
from open_knowledge_graph_embeddings_amd import hotpath as H
from open_knowledge_graph_embeddings_amd.checkpoint import load_reference_checkpoint, to_reference_checkpoint
from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep, GraphedTrainStep
import deterministic_reference as dr
from test_hip_parity import CASES, hp, test_g3_adagrad_steps as _default_g3, test_random_vs_oracle as _default_vs_oracle  # noqa: F401
from conftest import golden_names

N_ENT, N_REL, N_LIST = 40, 3, 33
PREFIX_ENTITIES = np.array([4, 9, 17, 22, 39])
BS = [1, 65, 130]
P_ENT, P_REL, SEED = 0.4, 0.2, 11


def _i32(a):
    return torch.tensor(np.asarray(a), dtype=torch.int32).cuda()


def _batch(rng, B, kind):
    """n_po = B // 2 po rows and the rest sp rows; candidates: "all" = the range 0 .. 39, "range" = rows 2 .. 39, "list" = 33
    ids drawn WITH repeats.  1-3 positives per row."""
    n_po = B // 2
    ent, rel = rng.choice(PREFIX_ENTITIES, B), rng.integers(0, N_REL, B)
    if kind == "list":
        cand = rng.integers(0, N_ENT, N_LIST)
        cand[5] = cand[20] = cand[0]                                     # one id three times at least
        n, how = N_LIST, dict(cand_ids=_i32(cand), cand_unique=False)
    else:
        first = 0 if kind == "all" else 2
        n, how = N_ENT - first, dict(cand_first=first, n_cand=N_ENT - first)
        cand = np.arange(first, N_ENT)
    labels = np.zeros((B, n), np.float32)
    for r in range(B):
        labels[r, rng.choice(n, size=int(rng.integers(1, 4)), replace=False)] = 1
    pos_row, pos_col = H.positives_from_dense(torch.from_numpy(labels).cuda())
    b = H.PrefixBatch(po_rel=_i32(rel[:n_po]) if n_po else None, po_obj=_i32(ent[:n_po]) if n_po else None,
                      sp_subj=_i32(ent[n_po:]), sp_rel=_i32(rel[n_po:]), pos_row=pos_row, pos_col=pos_col, **how)
    return b, np.concatenate([cand, ent]), rel


def _tables(d, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N_ENT, d, generator=g) * 0.2).cuda(), (torch.randn(N_REL, d, generator=g) * 0.2).cuda()


def _make(scorer, d, loss="bce", **kw):
    E, R = _tables(d)
    opts = dict(lr=0.3, weight_decay=0.0, eps=1e-8, input_dropout=P_ENT, relation_input_dropout=P_REL, seed=SEED,
                label_smoothing=0.1 if loss == "bce" else 0.0, loss=loss)
    opts.update(kw)
    return FusedTrainStep(E, R, scorer, **opts)


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


STATE = {"adagrad": ("E", "R", "sumE", "sumR"), "adam": ("E", "R", "mE", "vE", "mR", "vR", "adam_stateE", "adam_stateR")}


def _assert_same(a, b, la, lb, names=None, tag=None):
    for name in names or STATE[a.optimizer]:
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), (name, tag)
    assert len(la) == len(lb)
    for i, (x, y) in enumerate(zip(la, lb)):
        assert torch.equal(_bits(x), _bits(y)), ("loss", i, tag)


def _run(st, batches):
    """-> [(loss, grad_norm or None) per step], read after the run"""
    out = []
    for b in batches:
        loss = st.step(b).clone()
        out.append((loss, None if st.grad_norm is None else st.grad_norm.clone()))
    torch.cuda.synchronize()
    return [x[0] for x in out], [x[1] for x in out if x[1] is not None]


def _occurrence_rows(st, batch, step):
    """the rows an OKGE_TRAIN_ROW_GRADS call returns for this batch under the step's seed and masks at step count `step`"""
    d, n, B = st.E.shape[1], batch.n_candidates, batch.B
    gE, gR = torch.empty((n + B, d), device="cuda"), torch.empty((B, d), device="cuda")
    batch.set_dropout(H.dropout_specs(st.input_dropout, st.relation_input_dropout, st.seed, step))
    st.engine.forward_backward(st.E, st.R, st.scorer, batch, gE, gR, loss=st.loss, label_smoothing=st.label_smoothing, row_grads=True)
    torch.cuda.synchronize()
    return gE.cpu().numpy(), gR.cpu().numpy()


def _same_np(t, a):
    return np.array_equal(t.cpu().numpy().view(np.int32), a.view(np.int32))


# ------------------------------------------------------------------------------------------ the gradient itself
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["all", "range", "list"])
@pytest.mark.parametrize("scorer,d", [("complex", 6), ("distmult", 200)])
def test_forward_backward_leaves_the_densified_occurrence_rows(okge_lib, scorer, d, kind):
    for B in BS:
        rng = np.random.default_rng(B + d)
        b, ids_e, ids_r = _batch(rng, B, kind)
        assert B == 1 or (np.bincount(ids_r).max() > 12 and np.bincount(ids_e).max() > 6)
        st = _make(scorer, d, deterministic=True)
        st.steps = 1
        st.forward_backward(b)
        gE, gR = _occurrence_rows(st, b, 1)
        assert _same_np(st.dE, dr.densify(ids_e, gE, N_ENT)), (B, "dE")
        assert _same_np(st.dR, dr.densify(ids_r, gR, N_REL)), (B, "dR")
        assert float(st.dE.abs().max()) > 0 and float(st.dR.abs().max()) > 0


@pytest.mark.gpu
def test_accumulated_gradient_continues_each_rows_chain(okge_lib):
    for B in BS:
        rng = np.random.default_rng(B)
        (b1, e1, r1), (b2, e2, r2) = _batch(rng, B, "list"), _batch(rng, B, "range")
        st = _make("complex", 200, deterministic=True, accumulate=2)
        st.step(b1)                                       # first micro-batch of the window: stored, no optimizer step yet
        assert st._accumulated == 1
        st.steps += 1
        st.forward_backward(b2)                           # second: continued from what the tables hold
        g1, g2 = _occurrence_rows(st, b1, 1), _occurrence_rows(st, b2, 2)
        assert _same_np(st.dE, dr.densify(e2, g2[0], N_ENT, into=dr.densify(e1, g1[0], N_ENT))), B
        assert _same_np(st.dR, dr.densify(r2, g2[1], N_REL, into=dr.densify(r1, g1[1], N_REL))), B


# ------------------------------------------------------------------------------------------ against the row-sparse step
def _three_batches(B, seed):
    rng = np.random.default_rng(seed)
    return [_batch(rng, B, kind)[0] for kind in ("all", "list", "range")]


@pytest.mark.gpu
@pytest.mark.parametrize("d", [6, 200])
@pytest.mark.parametrize("loss", ["bce", "kl"])
@pytest.mark.parametrize("scorer", ["complex", "distmult"])
def test_three_steps_equal_the_sparse_step(okge_lib, scorer, loss, d):
    for B in BS:
        batches = _three_batches(B, 7 * B + d)
        det, sparse = _make(scorer, d, loss, deterministic=True), _make(scorer, d, loss, sparse=True)
        (ld, _), (ls, _) = _run(det, batches), _run(sparse, batches)
        _assert_same(det, sparse, ld, ls, tag=(B, "wd=0"))
        assert not det.dE.any() and not det.dR.any()                     # the sweeps cleared what the step stored
        if d == 200:
            det = _make(scorer, d, loss, deterministic=True, weight_decay=1e-10)
            lazy = _make(scorer, d, loss, sparse=True, weight_decay=1e-10, decay_window=4)
            (ld, _), (ls, _) = _run(det, batches), _run(lazy, batches)
            lazy.flush()
            torch.cuda.synchronize()
            _assert_same(det, lazy, ld, ls, tag=(B, "wd=1e-10"))


# ------------------------------------------------------------------------------------------ run to run
def _five_batches(B=65, kinds=("all", "list", "range", "list", "all")):
    rng = np.random.default_rng(5)
    return [_batch(rng, B, k)[0] for k in kinds]


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["adagrad", "adagrad_clip_accumulate", "adam", "kl"])
def test_two_runs_are_bit_identical(okge_lib, config):
    kw = {"adagrad": dict(weight_decay=1e-10),
          "adagrad_clip_accumulate": dict(weight_decay=1e-10, grad_clip=0.01, accumulate=2),
          "adam": dict(optimizer="adam", lr=0.01, weight_decay=1e-6, grad_clip=0.01),
          "kl": dict(loss="kl", weight_decay=1e-10)}[config]
    batches = _five_batches()
    a, b = _make("complex", 200, deterministic=True, **kw), _make("complex", 200, deterministic=True, **kw)
    (la, na), (lb, nb) = _run(a, batches), _run(b, batches)      # two runs, one after the other
    _assert_same(a, b, la, lb, names=STATE[a.optimizer] + ("dE", "dR"))
    assert len(na) == len(nb) == (len(batches) if "grad_clip" in kw else 0)
    for x, y in zip(na, nb):
        assert torch.equal(_bits(x), _bits(y))
    if "grad_clip" in kw:
        assert max(float(x) for x in na) > kw["grad_clip"]               # the clip was active, not a no-op
    assert float((a.E - _tables(200)[0]).abs().max()) > 0


@pytest.mark.gpu
def test_graphed_replays_equal_eager_steps(okge_lib):
    batches = _five_batches(kinds=("list",) * 3)
    cap = max(b.nnz for b in batches)
    eager = _make("complex", 200, deterministic=True, weight_decay=1e-10)
    le, _ = _run(eager, batches)
    inner = _make("complex", 200, deterministic=True, weight_decay=1e-10)
    gs = GraphedTrainStep(inner, batches[0], pos_capacity=cap)           # capture, then three replays
    lg = [gs.step(b).clone() for b in batches]
    torch.cuda.synchronize()
    _assert_same(eager, inner, le, lg, names=STATE["adagrad"] + ("dE", "dR"))


# ------------------------------------------------------------------------------------------ accuracy: the default step's bounds
class _DeterministicEngine:
    """stands in for the HotPath of tests/test_hip_parity.py: forward_backward is a deterministic FusedTrainStep's, everything
    else the real engine's -- so that file's own tests, bounds and all, judge the deterministic step"""

    def __init__(self, engine):
        self._engine = engine

    def __getattr__(self, name):
        return getattr(self._engine, name)

    def forward_backward(self, E, R, scorer, batch, dE, dR, loss="bce", label_smoothing=0.0, normalizer=None):
        st = FusedTrainStep(E, R, scorer, loss=loss, label_smoothing=label_smoothing, deterministic=True, engine=self._engine)
        out = st.forward_backward(batch, normalizer)
        dE += st.dE
        dR += st.dR
        return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", [CASES[i] for i in (1, 2, 4, 6, 7, 10)], ids=lambda c: f"{c[0]}-d{c[3]}-b{c[4]}+{c[5]}-{c[7]}")
def test_oracle_bounds_of_the_default_step(hp, case):      # noqa: F811
    _default_vs_oracle(_DeterministicEngine(hp), case)


@pytest.mark.gpu
@pytest.mark.parametrize("name", golden_names("g3_adagrad_")[:2])
def test_golden_adagrad_bounds_of_the_default_step(hp, name):      # noqa: F811
    _default_g3(_DeterministicEngine(hp), name)


# ------------------------------------------------------------------------------------------ checkpoints
@pytest.mark.gpu
@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
def test_resumed_run_is_bit_identical(okge_lib, optimizer):
    kw = dict(optimizer=optimizer, weight_decay=1e-10, lr=0.3 if optimizer == "adagrad" else 0.01)
    batches = _five_batches()
    whole = _make("complex", 200, deterministic=True, **kw)
    lw, _ = _run(whole, batches)
    first = _make("complex", 200, deterministic=True, **kw)
    l1, _ = _run(first, batches[:2])
    ckpt = to_reference_checkpoint(first)
    resumed = _make("complex", 200, deterministic=True, **kw)
    resumed.E.normal_()                                                   # (nothing of the fresh step's tables may survive)
    load_reference_checkpoint(resumed, ckpt)
    resumed.steps = first.steps                                          # the dropout counter (the checkpoint's training_steps)
    l2, _ = _run(resumed, batches[2:])
    _assert_same(whole, resumed, lw, l1 + l2)


# ------------------------------------------------------------------------------------------ refusals, and the default
@pytest.mark.gpu
def test_refusals_name_the_path_to_use(okge_lib):
    from open_knowledge_graph_embeddings_amd.sharded import ReplicaStep, ReplicaTrainStep
    E, R = _tables(8)
    with pytest.raises(ValueError, match="already bit-reproducible"):
        FusedTrainStep(E, R, "distmult", weight_decay=0.0, sparse=True, deterministic=True)
    with pytest.raises(NotImplementedError, match="l2_reg=0"):
        FusedTrainStep(E, R, "distmult", l2_reg=0.01, deterministic=True)
    wide = torch.zeros(N_ENT, 516, device="cuda")
    with pytest.raises(NotImplementedError, match="slot size 512"):
        FusedTrainStep(wide, torch.zeros(N_REL, 516, device="cuda"), "distmult", deterministic=True)
    with pytest.raises(NotImplementedError, match="deterministic=False"):
        ReplicaTrainStep(E, R, "distmult", deterministic=True)
    st = FusedTrainStep(E, R, "distmult", deterministic=True)
    with pytest.raises(NotImplementedError, match="deterministic=False"):
        ReplicaStep(st)
    big = H.PrefixBatch(sp_subj=_i32([4]), sp_rel=_i32([1]), pos_row=_i32([0]), pos_col=_i32([0]),
                        cand_ids=torch.zeros(2 ** 20, dtype=torch.int32, device="cuda"))
    with pytest.raises(N.OkgeError, match="2\\^20 occurrence rows"):
        st.step(big)
    assert not st.dE.any() and not st._rows                              # refused before anything was launched or allocated


@pytest.mark.gpu
def test_default_is_the_step_without_the_keyword(okge_lib):
    plain, off = _make("complex", 200, weight_decay=1e-10), _make("complex", 200, weight_decay=1e-10, deterministic=False)
    assert off.deterministic is False and plain.deterministic is False and plain.grad_norm is None
    # at most two contributions per row (B = 1 against the candidate range; two fp32 addends commute): batches on which the
    # default step's atomics are order-free, so two of its runs can be compared bit for bit
    rng = np.random.default_rng(2)
    single = [_batch(rng, 1, "range")[0] for _ in range(3)]
    (lp, _), (lo, _) = _run(plain, single), _run(off, single)
    _assert_same(plain, off, lp, lo, names=STATE["adagrad"] + ("dE", "dR"))
