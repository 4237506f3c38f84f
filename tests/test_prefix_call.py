"""hotpath.PrefixCall refilled in place: the step drivers keep ONE set of argument structs and refill it per batch, so a field
a fill forgets to write keeps the previous batch's value -- an `ids` pointer after a switch to a candidate range, the pointers of
a direction that became empty, a `step_dev` attached earlier.  After every fill of one persistent object the four structs must
be byte-equal to structs built fresh for that batch alone through the general fill (a PrefixBatch with dropout_specs).
No library call: the fills read data_ptr(), shapes and numbers only, so int32 host tensors stand in for device memory."""
import pytest
import torch

from open_knowledge_graph_embeddings_amd import hotpath as H

CPU = torch.device("cpu")


def _i32(*values):
    return torch.tensor(values, dtype=torch.int32)


E, R = torch.zeros((50, 16)), torch.zeros((12, 16))
E2, R2 = torch.zeros((40, 8)), torch.zeros((9, 8))
# (tables, scorer, po = (rel, obj), sp = (subj, rel), candidate ids, first, n, positives (row, col), candidate table,
#  dropout = (p_ent, p_rel, seed, step, step_dev))
BATCHES = {
    "both_directions_range": ((E, R, "complex"), (_i32(2, 3, 4), _i32(5, 6, 7)), (_i32(8, 9, 10, 11), _i32(5, 6, 7, 8)), None, 2, 48,
                              (_i32(0, 3, 6, 2), _i32(1, 4, 9, 40)), None, (0.3, 0.2, 1234, 1, None)),
    "no_po_id_list": ((E, R, "complex"), None, (_i32(12, 13), _i32(2, 3)), _i32(4, 9, 17, 30, 41), 2, 0,
                      (_i32(0, 1, 1), _i32(0, 2, 4)), None, (0.3, 0.2, 1234, 2, None)),
    "no_sp_range_fewer_positives": ((E, R, "complex"), (_i32(4, 5), _i32(20, 21)), None, None, 3, 47, (_i32(1), _i32(7)), None,
                                    (0.3, 0.2, 1234, 3, None)),
    "both_directions_step_dev": ((E, R, "complex"), (_i32(6), _i32(22)), (_i32(23, 24), _i32(7, 8)), None, 2, 48,
                                 (_i32(0, 2), _i32(3, 5)), None, (0.1, 0.4, 99, 4, _i32(4))),
    # beyond the four shapes of a training run: a candidate table (scoring), then other tables and no dropout at all
    "candidate_table": ((E, R, "distmult"), (_i32(1), _i32(2)), None, None, 0, 6, None, torch.zeros((6, 16)), (0.0, 0.0, 0, 0, None)),
    "other_tables_no_positives": ((E2, R2, "distmult"), None, (_i32(3), _i32(4)), _i32(5, 6), 0, 0, None, None, (0.0, 0.0, 0, 0, None)),
}


def _fresh(tables, po, sp, cand_ids, first, n, positives, cand_table, dropout):
    """structs that never held another batch, through the general fill"""
    batch = H.PrefixBatch(cand_ids=cand_ids, cand_first=first, n_cand=n, cand_table=cand_table).set_dropout(H.dropout_specs(*dropout))
    if po is not None:
        batch.po_rel, batch.po_obj = po
    if sp is not None:
        batch.sp_subj, batch.sp_rel = sp
    if positives is not None:
        batch.pos_row, batch.pos_col = positives
    call = H.PrefixCall()
    call.fill_tables(*tables, CPU)
    call.fill_batch(batch, CPU)
    return call


def _images(call):
    return {name: bytes(getattr(call, name)) for name in ("t", "pb", "c", "pos")}


def test_a_refilled_call_holds_nothing_of_the_batches_before():
    call, seen = H.PrefixCall(), []
    for name, (tables, po, sp, cand_ids, first, n, positives, cand_table, dropout) in BATCHES.items():
        call.fill_tables(*tables, CPU)
        call.fill_dropout(*dropout)
        call.fill_ids(*(po or (None, None)), *(sp or (None, None)), cand_ids, first, n, *(positives or (None, None)), cand_table)
        got, want = _images(call), _images(_fresh(tables, po, sp, cand_ids, first, n, positives, cand_table, dropout))
        for struct in want:
            assert got[struct] == want[struct], f"{name}: okge struct '{struct}' differs from a freshly built one"
        assert (call.B, call.n) == ((0 if po is None else po[0].numel()) + (0 if sp is None else sp[0].numel()),
                                    n if cand_ids is None else cand_ids.numel())
        seen.append(got)
    # (the sequence really moves every struct: a fill that wrote nothing would pass the comparison on equal batches only)
    for struct in ("t", "pb", "c", "pos"):
        assert len({image[struct] for image in seen}) >= 3


def test_the_fields_a_batch_does_not_use_read_as_none_and_zero():
    call = H.PrefixCall()
    for name in ("both_directions_step_dev", "candidate_table", "no_po_id_list"):
        tables, po, sp, cand_ids, first, n, positives, cand_table, dropout = BATCHES[name]
        call.fill_dropout(*dropout)
        call.fill_ids(*(po or (None, None)), *(sp or (None, None)), cand_ids, first, n, *(positives or (None, None)), cand_table)
    pb, c = call.pb, call.c
    assert pb.po_rel is None and pb.po_obj is None and pb.n_po == 0 and pb.n_sp == 2
    assert c.table is None and c.table_rows == 0 and c.ids == BATCHES["no_po_id_list"][3].data_ptr() and c.n == 5
    assert all(d.step_dev is None and d.keep is None and d.step == 2 for d in call.drops)
    assert [d.stream for d in call.drops] == list(H.STREAMS)


def test_fill_tables_refuses_what_the_general_path_refuses():
    call = H.PrefixCall()
    for bad_E in (E.double(), E.t()):
        with pytest.raises(H.N.OkgeError, match="embedding tables must be contiguous fp32 tensors on the engine's device"):
            call.fill_tables(bad_E, R, "complex", CPU)
