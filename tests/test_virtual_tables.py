"""The virtual-tables layout (virtual_tables.py) and the step skeleton on top of it, on the CPU: recording stand-ins for the
engine and the encoders, CPU tensors (the style of test_native_load.py::test_deferred_decay_bookkeeping_on_the_host)."""
import itertools

import pytest
import torch

from open_knowledge_graph_embeddings_amd import hotpath as H
from open_knowledge_graph_embeddings_amd import virtual_tables as VT

SHAPES = [s for s in itertools.product((1, 5, 64), (0, 1, 7), (0, 1, 9)) if s[1] + s[2] > 0]


def i32(*a):
    return torch.arange(*a, dtype=torch.int32)


@pytest.mark.parametrize("N,n_po,n_sp", SHAPES)
def test_layout_round_trip_and_literal_formulas(N, n_po, n_sp):
    """rows written through the five row ranges come back through the position batch's indices, each call its own rows; the
    indices are the formulas EV = [candidates | po objects | sp subjects], RV = [po relations | sp relations] written out"""
    B = n_po + n_sp
    cand, po_rel, po_obj, sp_subj, sp_rel = VT.row_ranges(N, n_po, n_sp)
    EV, RV = torch.full((N + B, 2), -1.0), torch.full((B, 2), -1.0)
    for tag, (table, rows) in enumerate(((EV, cand), (RV, po_rel), (EV, po_obj), (EV, sp_subj), (RV, sp_rel))):
        n = rows.stop - rows.start
        assert (table[rows] == -1).all()                             # no two calls share a row
        table[rows] = torch.stack([torch.full((n,), float(tag)), torch.arange(n, dtype=torch.float32)], 1)
    assert (EV >= 0).all() and (RV >= 0).all()                       # ... and together they cover both tables
    prow, pcol = i32(3), i32(3)
    vt = VT.VirtualTables("cpu")
    vb = vt.batch(N, n_po, n_sp, prow, pcol)
    assert (vb.cand_first, vb.n_cand, vb.cand_ids, vb.n_po, vb.n_sp) == (0, N, None, n_po, n_sp)
    assert vb.pos_row is prow and vb.pos_col is pcol
    assert all(getattr(vb, f"drop_{k}") is H.NO_DROP for k in ("cand", "po_ent", "po_rel", "sp_ent", "sp_rel"))
    want = {"po_rel": (RV, 1, i32(0, n_po)), "po_obj": (EV, 2, i32(N, N + n_po)),
            "sp_subj": (EV, 3, i32(N + n_po, N + B)), "sp_rel": (RV, 4, i32(n_po, B))}
    for name, (table, tag, literal) in want.items():
        idx = getattr(vb, name)
        if literal.numel() == 0:
            assert idx is None
            continue
        assert idx.dtype == torch.int32 and torch.equal(idx, literal)
        got = table[idx.long()]
        assert (got[:, 0] == tag).all() and torch.equal(got[:, 1], torch.arange(literal.numel(), dtype=torch.float32))
    assert (EV[:N, 0] == 0).all() and torch.equal(EV[:N, 1], torch.arange(N, dtype=torch.float32))     # candidates: rows 0..N-1
    again = vt.batch(N, n_po, n_sp, prow, pcol)
    assert all((getattr(vb, k) is None and getattr(again, k) is None) or getattr(vb, k).data_ptr() == getattr(again, k).data_ptr()
               for k in want)
    drops = H.dropout_specs(0.1, 0.2, 3, 4)
    vb = vt.batch(N, n_po, n_sp, prow, pcol, drops)
    assert (vb.drop_cand, vb.drop_po_ent, vb.drop_po_rel, vb.drop_sp_ent, vb.drop_sp_rel) == drops


def test_encode_calls_follow_the_reference_order():
    b = H.PrefixBatch(po_rel=i32(10, 13), po_obj=i32(20, 23), sp_subj=i32(30, 34), sp_rel=i32(40, 44), cand_first=2, n_cand=6)
    calls = VT.encode_calls(b)
    assert [c[0] for c in calls] == [False, True, False, False, True]
    assert [c[1] for c in calls] == [None, b.po_rel, b.po_obj, b.sp_subj, b.sp_rel] and [c[2] for c in calls] == [2, 0, 0, 0, 0]
    assert [c[3] for c in calls] == [slice(0, 6), slice(0, 3), slice(6, 9), slice(9, 13), slice(3, 7)]


class Engine:
    """records HotPath.forward_backward"""

    def __init__(self, log):
        self.log, self.calls = log, []

    def forward_backward(self, E, R, scorer, batch, dE, dR, **kw):
        self.log.append("fused")
        self.calls.append(dict(E=E, R=R, scorer=scorer, batch=batch, dE=dE, dR=dR, **kw))
        return kw["loss_out"]


def batch_of(N, n_po, n_sp):
    return H.PrefixBatch(po_rel=i32(n_po) if n_po else None, po_obj=i32(n_po) if n_po else None, sp_subj=i32(n_sp) if n_sp else None,
                         sp_rel=i32(n_sp) if n_sp else None, pos_row=i32(2), pos_col=i32(2), cand_first=2, n_cand=N)


def specs(vb):
    return [(d.p, d.seed, d.stream, d.step, d.step_dev) for d in (vb.drop_cand, vb.drop_po_ent, vb.drop_po_rel, vb.drop_sp_ent, vb.drop_sp_rel)]


def check_fused_call(call, st, shape, p_ent, p_rel, step, bn):
    N, n_po, n_sp = shape
    B = n_po + n_sp
    assert call["grads_zero"] is True and call["distinct_prefix_rows"] is True
    assert call["loss"] == "bce" and call["loss_out"] is st.loss_out and call["scorer"] == "complex"
    assert specs(call["batch"]) == [(p_ent, 11, H.STREAM_CAND, step, None), (p_ent, 11, H.STREAM_PO_ENT, step, None),
                                    (p_rel, 11, H.STREAM_PO_REL, step, None), (p_ent, 11, H.STREAM_SP_ENT, step, None),
                                    (p_rel, 11, H.STREAM_SP_REL, step, None)]
    EV, EX, dEV, RV, RX, dRV = st.tables.buffers(N, n_po, n_sp, 4)
    assert call["E"].data_ptr() == (EV if bn else EX).data_ptr() and call["R"].data_ptr() == (RV if bn else RX).data_ptr()
    assert EV.data_ptr() != EX.data_ptr() and call["dE"].data_ptr() == dEV.data_ptr() and call["dR"].data_ptr() == dRV.data_ptr()
    assert call["E"].shape == call["dE"].shape == (N + B, 4) and call["R"].shape == call["dR"].shape == (B, 4)
    vb = call["batch"]
    assert (vb.cand_first, vb.n_cand, vb.n_po, vb.n_sp) == (0, N, n_po, n_sp)


def drive(st, eng, log, p_ent, p_rel, bn, order=("encode", "fused", "backward")):
    """two steps of one shape, then a larger one: flags, specs, tables, call order, index reuse, buffer growth"""
    small, large = (5, 1, 2), (64, 7, 9)
    assert st.forward_backward(batch_of(*small)) is st.loss_out
    st.forward_backward(batch_of(*small))
    assert log == list(order) * 2 and st.steps == 2
    for step, call in enumerate(eng.calls, 1):
        check_fused_call(call, st, small, p_ent, p_rel, step, bn)
    a, b = (c["batch"] for c in eng.calls)
    for k in ("po_rel", "po_obj", "sp_subj", "sp_rel"):
        assert getattr(a, k).data_ptr() == getattr(b, k).data_ptr()
    assert eng.calls[0]["dE"].data_ptr() == eng.calls[1]["dE"].data_ptr()
    st.forward_backward(batch_of(*large), normalizer=3.0)
    check_fused_call(eng.calls[2], st, large, p_ent, p_rel, 3, bn)
    assert eng.calls[2]["normalizer"] == 3.0 and eng.calls[2]["dE"].data_ptr() != eng.calls[0]["dE"].data_ptr()
    st.forward_backward(batch_of(64, 0, 9))                             # one direction empty
    vb = eng.calls[3]["batch"]
    assert vb.po_rel is None and vb.po_obj is None and torch.equal(vb.sp_subj, i32(64, 73)) and torch.equal(vb.sp_rel, i32(0, 9))


@pytest.mark.parametrize("bn", [False, True])
def test_token_pooled_step_hands_the_engine_the_virtual_tables(bn):
    from open_knowledge_graph_embeddings_amd.token_pooled import TokenPooledTrainStep, TokenSlot
    log = []

    class Pool:
        def encode_calls(self, calls, training):
            log.append("encode")
            self.encoded = [(c[0], c[3], c[4].data_ptr(), c[5].data_ptr(), c[6] is not None) for c in calls if c[3] > 0]

        def backward_calls(self, calls):
            log.append("backward")
            self.backwarded = [(c[0], c[3], c[4].data_ptr(), c[5].data_ptr(), c[6] is not None) for c in calls if c[3] > 0]

    tok = torch.zeros((80, 3), dtype=torch.int32)
    e, r = TokenSlot(torch.zeros(8, 4), tok, "sum", bn), TokenSlot(torch.zeros(6, 4), tok, "sum", bn)
    eng = Engine(log)
    st = TokenPooledTrainStep(e, r, "complex", dropout=0.25, seed=11, engine=eng)
    st.pool = pool = Pool()
    assert st.step_dev is None and st.decay_window == 1
    drive(st, eng, log, 0.25, 0.25, bn)
    # the last batch (64, 0, 9), its non-empty calls: candidates and sp subjects on the entity slot, sp relations on the relation slot
    EV, EX, dEV, RV, RX, dRV = st.tables.buffers(64, 0, 9, 4)
    row = EV.stride(0) * EV.element_size()
    assert pool.encoded == [(e, 64, EX.data_ptr(), (EV if bn else EX).data_ptr(), bn),
                            (e, 9, EX.data_ptr() + 64 * row, (EV if bn else EX).data_ptr() + 64 * row, bn),
                            (r, 9, RX.data_ptr(), (RV if bn else RX).data_ptr(), bn)]
    assert pool.backwarded == [(e, 64, EX.data_ptr(), dEV.data_ptr(), bn), (e, 9, EX.data_ptr() + 64 * row, dEV.data_ptr() + 64 * row, bn),
                               (r, 9, RX.data_ptr(), dRV.data_ptr(), bn)]


@pytest.mark.parametrize("bn", [False, True])
def test_lstm_step_hands_the_engine_the_virtual_tables(bn):
    from open_knowledge_graph_embeddings_amd.lstm import LSTMSlot, LSTMTrainStep
    log = []

    class Pass:
        def __init__(self):
            self.seen = []

        def encode(self, slot, calls, training, raw, out):
            log.append("encode")
            self.seen.append(("encode", slot, [(c[1], c[2]) for c in calls], training, raw.data_ptr(), out.data_ptr(), tuple(raw.shape)))

        def backward(self, slot, calls, raw, d_out, dW, dlstm, d_bn):
            log.append("backward")
            self.seen.append(("backward", slot, [(c[1], c[2]) for c in calls], raw.data_ptr(), d_out.data_ptr(), dW is slot.dW,
                              dlstm is slot.dlstm, d_bn is (slot.d_bn if bn else None)))

    def slot(vocab):
        d = 4
        lstm = [torch.zeros(4 * d, d), torch.zeros(4 * d, d), torch.zeros(4 * d), torch.zeros(4 * d)]
        return LSTMSlot(torch.zeros(vocab, d), torch.zeros((80, 3), dtype=torch.int32), lstm,
                        (torch.ones(d), torch.zeros(d)) if bn else None, (torch.zeros(d), torch.ones(d)) if bn else None)
    e, r = slot(8), slot(6)
    assert [tuple(g.shape) for g in e.dlstm] == [(16, 4), (16, 4), (16,), (16,)] and e.dlstm[1].data_ptr() == e.d_flat[64:].data_ptr()
    eng = Engine(log)
    st = LSTMTrainStep(e, r, "complex", dropout=0.25, relation_dropout=0.5, seed=11, engine=eng)
    st.passes = pe, pr = Pass(), Pass()
    assert st.step_dev is None and st.decay_window == 1
    drive(st, eng, log, 0.25, 0.5, bn, order=["encode", "encode", "fused", "backward", "backward"])      # one pass per slot each way
    # the first batch (5, 1, 2): the three entity calls share one pass over EV's rows, the two relation calls one over RV's
    first = eng.calls[0]
    assert pe.seen[0][:4] == ("encode", e, [(2, 5), (0, 1), (0, 2)], True) and pe.seen[0][6] == (8, 4)
    assert pr.seen[0][:4] == ("encode", r, [(0, 1), (0, 2)], True) and pr.seen[0][6] == (3, 4)
    assert pe.seen[0][5 if bn else 4] == first["E"].data_ptr() and pr.seen[0][5 if bn else 4] == first["R"].data_ptr()
    assert (pe.seen[0][4] != pe.seen[0][5]) and (pr.seen[0][4] != pr.seen[0][5])
    assert pe.seen[1] == ("backward", e, [(2, 5), (0, 1), (0, 2)], pe.seen[0][4], first["dE"].data_ptr(), True, True, True)
    assert pr.seen[1] == ("backward", r, [(0, 1), (0, 2)], pr.seen[0][4], first["dR"].data_ptr(), True, True, True)
    # the last one (64, 0, 9): the empty po calls are left out
    assert pe.seen[-2][2] == [(2, 64), (0, 9)] and pr.seen[-2][2] == [(0, 9)] and pe.seen[-2][-1] == (73, 4)
