"""The prefix backward's scatter (prefix_backward_vec_kernel, csrc/okge_misc.hip): on the atomic path the lead lane of a 4-lane
column group forms the four columns of a gradient row and every lane of the group adds ONE of them, so that a wave adds 64
consecutive floats per instruction (csrc/okge_prefix_device.h, profiles/step_tail.md).  The same floats reach the same
addresses as when the lead lane added all four; the store paths (row segments, distinct prefix rows) keep the lead lane's stores.

Through HotPath.prefix_backward (one dQ block: the NB = 1 instance), atomics against the segmented path
(sharded.make_row_segments: rows stored, then summed per id in a fixed order):
  * distinct ids -- one add per destination: bit for bit, and two runs identical;
  * repeated ids -- against a float64 restatement of the chain rule and the scatter, tests/lstm_reference.band_check at its default
    factors (per magnitude band: max error <= 3 x, rms error <= 1.6 x the fp32 restatement's), once with a numpy fp32 restatement
    (sequential adds) and once with the segmented path's result as the fp32 yardstick.
Through the fused step (32 dQ slabs: the NB = 8 instance), atomics against the step's own occurrence rows (OKGE_TRAIN_ROW_GRADS:
the same kernel stores every batch row's gradient rows instead of adding them), summed per id in float64 and in fp32."""
import numpy as np
import pytest
import torch

from lstm_reference import band_check
from oracle import kge_oracle as ko
from test_dq_split import SEED

STEP, P = 3, 0.4


def engine():
    from open_knowledge_graph_embeddings_amd import hotpath as H
    return H.HotPath("cuda:0")


def prefix_ids(rng, mode, B, n_po, n_ent, n_rel, ent_lo=2):
    """-> (rel[B], ent[B]) of the batch rows, po rows first"""
    if mode == "distinct":
        return 2 + rng.permutation(n_rel - 2)[:B], ent_lo + rng.permutation(n_ent - ent_lo)[:B]
    if mode == "one_rel":
        return np.full(B, 5), ent_lo + rng.permutation(n_ent - ent_lo)[:B]
    if mode == "one_ent":
        return 2 + rng.permutation(n_rel - 2)[:B], np.full(B, ent_lo + 7)
    # FB15k-237-like: a few frequent relations and many rare ones, every third entity, with repeats
    w = 1.0 / np.arange(1, n_rel - 1) ** 1.2
    return 2 + rng.choice(n_rel - 2, size=B, p=w / w.sum()), ent_lo + 3 * rng.integers(0, max(2, (n_ent - ent_lo) // 3), B)


def masks(stream_ent, stream_rel, n, d):
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(P))
    return ((ko.dropout_keep_mask(SEED, stream_ent, STEP, n, d, P) * scale).astype(np.float32),
            (ko.dropout_keep_mask(SEED, stream_rel, STEP, n, d, P) * scale).astype(np.float32))


def chain_rule(scorer, e, r, me, mr, dq, sp, e_masked, dt):
    """the gradient rows of every batch row: e / r the table rows (e already masked when e_masked), me / mr keep x scale"""
    e, r, me, mr, dq = (x.astype(dt) for x in (e, r, me, mr, dq))
    ev = e if e_masked else e * me
    rv = r * mr
    if scorer == "distmult":
        return dq * rv * me, dq * ev * mr
    h = e.shape[1] // 2
    q1, q2, e1, e2, r1, r2 = dq[:, :h], dq[:, h:], ev[:, :h], ev[:, h:], rv[:, :h], rv[:, h:]
    s = np.where(sp[:, None], dt(1), dt(-1))            # sp rows conjugate the relation, po rows the entity
    de = np.concatenate([q1 * r1 + s * (q2 * r2), q2 * r1 - s * (q1 * r2)], 1)
    dr = np.concatenate([q1 * e1 + q2 * e2, s * (q2 * e1 - q1 * e2)], 1)
    return de * me, dr * mr


def scatter(rows, ids, n, dt):
    out = np.zeros((n, rows.shape[1]), dt)
    np.add.at(out, ids, rows.astype(dt))
    return out


def prefix_case(scorer, d, B, mode, seed, shard=None):
    """one okge_prefix_backward call with float atomics and one by row segments -> the touched rows of
    (atomics dE, dR), (segments dE, dR), (float64 dE, dR), (numpy fp32 dE, dR)"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    from open_knowledge_graph_embeddings_amd.sharded import make_row_segments
    rng = np.random.default_rng(seed)
    hp = engine()
    dev = hp.device
    n_ent, n_rel = 300, 80
    lo, hi = shard if shard else (0, n_ent)
    E = (rng.standard_normal((n_ent, d)) * 0.1).astype(np.float32)
    R = (rng.standard_normal((n_rel, d)) * 0.1).astype(np.float32)
    n_po = B // 2
    rel, ent = prefix_ids(rng, mode, B, n_po, n_ent, n_rel)
    sp = np.arange(B) >= n_po
    i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(dev)            # noqa: E731
    batch = H.PrefixBatch(po_rel=i32(rel[:n_po]) if n_po else None, po_obj=i32(ent[:n_po]) if n_po else None,
                          sp_subj=i32(ent[n_po:]), sp_rel=i32(rel[n_po:]), cand_first=2, n_cand=n_ent - 2)
    _, batch.drop_po_ent, batch.drop_po_rel, batch.drop_sp_ent, batch.drop_sp_rel = H.dropout_specs(P, P, SEED, STEP)
    me, mr = np.ones((B, d), np.float32), np.ones((B, d), np.float32)
    if n_po:
        me[:n_po], mr[:n_po] = masks(H.STREAM_PO_ENT, H.STREAM_PO_REL, n_po, d)
    me[n_po:], mr[n_po:] = masks(H.STREAM_SP_ENT, H.STREAM_SP_REL, B - n_po, d)
    rows, ld = hp.query_shape(B, d)
    dq = np.zeros((rows, ld), np.float32)
    dq[:B, :d] = (rng.standard_normal((B, d)) * 1e-3).astype(np.float32)
    owned = (ent >= lo) & (ent < hi)
    ent_rows = None
    if shard:                              # the sharded call: every rank holds the masked entity rows of ALL prefixes
        er = np.zeros((rows, ld), np.float32)
        er[:B, :d] = E[ent] * me
        ent_rows = torch.from_numpy(er).to(dev)
    Et, Rt, dQ = torch.from_numpy(E[lo:hi].copy()).to(dev), torch.from_numpy(R).to(dev), torch.from_numpy(dq).to(dev)
    sh = H.Shard(lo, hi, 0)
    segs = make_row_segments(rel[:n_po], ent[:n_po], ent[n_po:], rel[n_po:], dev, min_rows=0, min_rows_per_relation=0.0)
    assert segs is not None and segs.rel is not None and segs.ent is not None
    out = []
    for plan in (None, None, segs):
        dE, dR = torch.zeros_like(Et), torch.zeros_like(Rt)
        hp.prefix_backward(Et, Rt, scorer, batch, sh, dQ, ent_rows, dE, dR, rel_segments=plan)
        torch.cuda.synchronize()
        out.append((dE.cpu(), dR.cpu()))
    e_in = (E[ent] * me) if shard else E[ent]
    rel_live = np.ones(B, bool) if shard else owned            # (without the exchanged rows a rank skips rows it does not own)
    want = []
    for dt in (np.float64, np.float32):
        de, dr = chain_rule(scorer, e_in, R[rel], me, mr, dq[:B, :d], sp, bool(shard), dt)
        want.append((scatter(de[owned], ent[owned] - lo, hi - lo, dt), scatter(dr[rel_live], rel[rel_live], n_rel, dt)))
    te, tr = np.unique(ent[owned] - lo), np.unique(rel[rel_live])
    untouched_e, untouched_r = np.ones(hi - lo, bool), np.ones(n_rel, bool)
    untouched_e[te], untouched_r[tr] = False, False
    for dE, dR in out:
        assert not dE[torch.from_numpy(untouched_e)].any() and not dR[torch.from_numpy(untouched_r)].any(), "rows no prefix names"
    pick = lambda pair: (np.asarray(pair[0])[te], np.asarray(pair[1])[tr])               # noqa: E731
    return [pick((a.numpy(), b.numpy())) for a, b in out] + [pick(w) for w in want]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def check_prefix(scorer, d, B, mode, seed, shard=None):
    name = f"{scorer} d={d} B={B} {mode}" + (f" shard={shard}" if shard else "")
    first, second, seg, want, want32 = prefix_case(scorer, d, B, mode, seed, shard)
    for i, what in enumerate(("dE", "dR")):
        assert np.abs(first[i]).max() > 0, (name, what)
        if mode == "distinct":
            assert same_bits(first[i], seg[i]), (name, what, "atomics against row segments")
            assert same_bits(first[i], second[i]), (name, what, "two runs")
        r32 = band_check(f"{name} {what} vs numpy fp32", first[i], want[i], want32[i])
        rsg = band_check(f"{name} {what} vs row segments", first[i], want[i], seg[i].astype(np.float64))
        print(f"{name} {what}: worst (max, rms) error ratio {r32[0]:.3f} {r32[1]:.3f} vs numpy fp32, {rsg[0]:.3f} {rsg[1]:.3f} vs row segments")


# d = 200: only 25 of the 32 column groups are active; DistMult d = 512: blockIdx.y column chunks
SHAPES = [("complex", 8), ("complex", 16), ("complex", 200), ("complex", 208), ("distmult", 4), ("distmult", 200), ("distmult", 512)]


@pytest.mark.gpu
@pytest.mark.parametrize("scorer,d", SHAPES)
def test_distinct_ids_equal_row_segments_bit_for_bit(scorer, d, okge_lib):
    for B in (1, 65):                       # B = 1: n_po = 0
        check_prefix(scorer, d, B, "distinct", 100 * d + B)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["one_rel", "one_ent", "fb"])
@pytest.mark.parametrize("scorer,d", SHAPES)
def test_repeated_ids_within_the_fp32_band(scorer, d, mode, okge_lib):
    check_prefix(scorer, d, 65, mode, 7 * d + len(mode))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["distinct", "fb"])
@pytest.mark.parametrize("scorer,d", [("complex", 200), ("distmult", 512)])
def test_sharded_call_with_rows_it_does_not_own(scorer, d, mode, okge_lib):
    """rows [100, 220) of the entity table live here: the relation gradient takes every batch row, the entity gradient only the
    owned ones"""
    check_prefix(scorer, d, 65, mode, 31 * d + len(mode), shard=(100, 220))


# ------------------------------------------------------------------------------------------------------------ the fused step
def step_case(scorer, d, B, mode, seed, n_po=None):
    """one fused step with float atomics (twice) and one that stores its occurrence rows -> the prefix rows of dE and dR:
    (atomics, atomics again, float64 sum of the occurrence rows, their sequential fp32 sum)"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    rng = np.random.default_rng(seed)
    hp = engine()
    dev = hp.device
    N, n_rel = 600, 80                      # ten 64-candidate tiles: the dQ product leaves 32 slabs
    n_ent = N + 2 + 100
    Et = torch.from_numpy((rng.standard_normal((n_ent, d)) * 0.1).astype(np.float32)).to(dev)
    Rt = torch.from_numpy((rng.standard_normal((n_rel, d)) * 0.1).astype(np.float32)).to(dev)
    n_po = B // 2 if n_po is None else n_po
    rel, ent = prefix_ids(rng, mode, B, n_po, n_ent, n_rel, ent_lo=N + 2)      # prefix entities behind the candidate range
    i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(dev)            # noqa: E731
    y = np.zeros((B, N), bool)
    for r in range(B):
        y[r, rng.choice(N, size=int(rng.integers(1, 4)), replace=False)] = True
    col, row = np.nonzero(y.T)
    batch = H.PrefixBatch(po_rel=i32(rel[:n_po]) if n_po else None, po_obj=i32(ent[:n_po]) if n_po else None,
                          sp_subj=i32(ent[n_po:]), sp_rel=i32(rel[n_po:]), pos_row=i32(row), pos_col=i32(col), cand_first=2, n_cand=N)
    batch.drop_cand, batch.drop_po_ent, batch.drop_po_rel, batch.drop_sp_ent, batch.drop_sp_rel = H.dropout_specs(P, P, SEED, STEP)
    runs = []
    for _ in range(2):
        dE, dR = torch.zeros_like(Et), torch.zeros_like(Rt)
        hp.forward_backward(Et, Rt, scorer, batch, dE, dR, grads_zero=True)
        torch.cuda.synchronize()
        runs.append((dE.cpu().numpy(), dR.cpu().numpy()))
    rE, rR = torch.empty((N + B, d), device=dev), torch.empty((B, d), device=dev)
    hp.forward_backward(Et, Rt, scorer, batch, rE, rR, grads_zero=True, row_grads=True)
    torch.cuda.synchronize()
    rows_e, rows_r = rE[N:].cpu().numpy(), rR.cpu().numpy()
    te, tr = np.unique(ent), np.unique(rel)
    sums = [(scatter(rows_e, ent, n_ent, dt)[te], scatter(rows_r, rel, n_rel, dt)[tr]) for dt in (np.float64, np.float32)]
    untouched = np.ones(n_ent, bool)
    untouched[te] = False
    untouched[2:N + 2] = False
    assert not runs[0][0][untouched].any()
    return [(a[te], b[tr]) for a, b in runs] + sums


@pytest.mark.gpu
@pytest.mark.parametrize("scorer,d", [("complex", 200), ("complex", 208), ("distmult", 200)])
def test_fused_step_adds_its_occurrence_rows(scorer, d, okge_lib):
    for B, mode, n_po in ((65, "distinct", None), (65, "distinct", 0), (1, "distinct", None), (65, "one_rel", None), (65, "one_ent", None),
                          (65, "fb", None)):
        name = f"step {scorer} d={d} B={B} {mode} n_po={n_po}"
        first, second, want, want32 = step_case(scorer, d, B, mode, 13 * d + B + len(mode), n_po)
        for i, what in enumerate(("dE", "dR")):
            assert np.abs(first[i]).max() > 0, (name, what)
            if mode == "distinct":
                assert same_bits(first[i], want32[i]), (name, what, "atomics against the stored rows")
                assert same_bits(first[i], second[i]), (name, what, "two runs")
            r = band_check(f"{name} {what}", first[i], want[i], want32[i])
            print(f"{name} {what}: worst (max, rms) error ratio {r[0]:.3f} {r[1]:.3f}")
