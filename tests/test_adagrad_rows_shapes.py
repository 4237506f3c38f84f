"""okge_adagrad_rows against the existing dense okge_adagrad_step2 at weight_decay = 0, fed the densified gradient that
tests/sparse_reference.py coalesces (per id, ascending position, sequential fp32): tables and accumulators BIT FOR BIT, every
untouched row and rows 0, 1 and last included.

The coalescing sum is plain fp32 addition in a fixed order, so the NumPy statement and the kernel agree exactly; the update is
compared kernel against kernel (both correctly rounded, the same operation order)."""
import numpy as np
import pytest
import torch

from open_knowledge_graph_embeddings_amd import _native as N
from open_knowledge_graph_embeddings_amd import hotpath as H
import sparse_reference as sr

ROWS = 97            # table rows (the all-distinct pattern takes n + 2 rows when n is larger)
NS = [0, 1, 63, 64, 65, 4097]
ROW_LENS = [1, 4, 5, 200, 512]
LR, EPS = 0.3, 1e-8


def _ids(pattern, n, rows, rng):
    if pattern == "distinct":
        return rng.permutation(rows)[:n].astype(np.int32)
    if pattern == "equal":
        return np.full(n, 41, np.int32)
    out = []                                        # runs of 3-7 repeats, the same id coming back later in the list
    while sum(map(len, out)) < n:
        out.append(np.full(rng.integers(3, 8), rng.integers(0, rows)))
    ids = np.concatenate(out + [np.zeros(0, np.int64)])[:n].astype(np.int32)
    if n > 2:
        ids[0], ids[1], ids[-1] = 0, 1, rows - 1    # rows 0, 1 and last are touched ...
    return ids


def _run_both(hp, p0, s0, ids, g, second=None):
    """-> ((p, s) by okge_adagrad_rows, (p, s) by the dense kernel on the coalesced gradient)"""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    p, s = dev(p0), dev(s0)
    args = (p, s, dev(ids), dev(g).reshape(len(ids), p0.shape[1]))
    if second is None:
        hp.adagrad_rows(*args, LR, EPS)
    else:
        hp.adagrad_rows(*args, LR, EPS, second=second)
    dense, _ = sr.coalesce(ids, g, p0.shape[0])
    pd, sd, gd = dev(p0), dev(s0), dev(dense)
    dummy = [torch.zeros(4, device="cuda") for _ in range(3)]
    hp.adagrad2(pd, gd, sd, *dummy, LR, 0.0, EPS, zero_grad=False)
    return (p, s), (pd, sd)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("row_len", ROW_LENS)
@pytest.mark.parametrize("pattern", ["distinct", "equal", "runs"])
def test_rows_update_equals_dense_step(okge_lib, pattern, row_len):
    hp = H.HotPath("cuda:0")
    rng = np.random.default_rng(ROW_LENS.index(row_len) * 10 + len(pattern))
    for n in NS:
        for warm in (False, True):
            rows = max(ROWS, n + 2) if pattern == "distinct" else ROWS
            p0 = (rng.standard_normal((rows, row_len)) * 0.1).astype(np.float32)
            s0 = (rng.random((rows, row_len)).astype(np.float32) + 1e-3) if warm else np.zeros((rows, row_len), np.float32)
            ids = _ids(pattern, n, rows, rng)
            g = (rng.standard_normal((n, row_len)) * 1e-2).astype(np.float32)
            (p, s), (pd, sd) = _run_both(hp, p0, s0, ids, g)
            tag = (pattern, row_len, n, warm)
            assert _same_bits(p, pd) and _same_bits(s, sd), tag
            untouched = np.setdiff1d(np.arange(rows), ids)
            assert np.array_equal(p.cpu().numpy()[untouched], p0[untouched]) and np.array_equal(s.cpu().numpy()[untouched], s0[untouched]), tag
            if n:
                assert not np.array_equal(p.cpu().numpy()[ids[0]], p0[ids[0]]), tag
            if pattern == "runs" and n > 2:
                for r in (0, 1, rows - 1):
                    assert not np.array_equal(p.cpu().numpy()[r], p0[r]), tag
            if pattern == "equal" and n:                                  # ... and here rows 0, 1 and last are NOT: bit-unchanged
                for r in (0, 1, rows - 1):
                    assert np.array_equal(p.cpu().numpy()[r], p0[r]) and np.array_equal(s.cpu().numpy()[r], s0[r]), tag


@pytest.mark.gpu
def test_two_tensors_share_the_launches_and_strided_rows(okge_lib):
    """entity- and relation-shaped tensors in one call (different n, row counts, lane counts), and gradient rows read through a
    leading dimension (a column slice of a wider buffer)"""
    hp = H.HotPath("cuda:0")
    rng = np.random.default_rng(5)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    pa0, sa0 = (rng.standard_normal((ROWS, 200)) * 0.1).astype(np.float32), rng.random((ROWS, 200)).astype(np.float32)
    pb0, sb0 = (rng.standard_normal((11, 200)) * 0.1).astype(np.float32), np.zeros((11, 200), np.float32)
    ia, ib = _ids("runs", 2100, ROWS, rng), rng.integers(0, 11, 77).astype(np.int32)
    ga = (rng.standard_normal((2100, 200)) * 1e-2).astype(np.float32)
    wide = (rng.standard_normal((77, 208)) * 1e-2).astype(np.float32)
    gb_dev = dev(wide)[:, :200]                                                 # ld_g = 208
    pb, sb = dev(pb0), dev(sb0)
    (pa, sa), (pad, sad) = _run_both(hp, pa0, sa0, ia, ga, second=(pb, sb, dev(ib), gb_dev))
    assert _same_bits(pa, pad) and _same_bits(sa, sad)
    dense, _ = sr.coalesce(ib, wide[:, :200], 11)
    pbd, sbd, gbd = dev(pb0), dev(sb0), dev(dense)
    dummy = [torch.zeros(4, device="cuda") for _ in range(3)]
    hp.adagrad2(pbd, gbd, sbd, *dummy, LR, 0.0, EPS, zero_grad=False)
    assert _same_bits(pb, pbd) and _same_bits(sb, sbd)


@pytest.mark.gpu
def test_out_of_range_ids_are_skipped_and_counted(okge_lib):
    hp = H.HotPath("cuda:0")
    rng = np.random.default_rng(8)
    assert N.id_errors() == 0
    p0 = (rng.standard_normal((ROWS, 64)) * 0.1).astype(np.float32)
    s0 = rng.random((ROWS, 64)).astype(np.float32)
    ids = _ids("runs", 130, ROWS, rng)
    ids[7], ids[40], ids[99] = ROWS, -1, 2 ** 31 - 1
    g = (rng.standard_normal((130, 64)) * 1e-2).astype(np.float32)
    (p, s), (pd, sd) = _run_both(hp, p0, s0, ids, g)                    # (the NumPy coalescing skips the same three rows)
    torch.cuda.synchronize()
    assert N.id_errors() == 3                                           # read AND reset: the id-guard fixture expects zero afterwards
    assert _same_bits(p, pd) and _same_bits(s, sd)


@pytest.mark.gpu
def test_size_limit_and_workspace(okge_lib):
    assert okge_lib.okge_adagrad_rows_workspace_bytes(0, 0) == 0
    assert okge_lib.okge_adagrad_rows_workspace_bytes(2 ** 20, 2 ** 20) == 4 * 8 * 2 ** 20
    assert okge_lib.okge_adagrad_rows_workspace_bytes(2 ** 20 + 1, 0) == 0
    t = N.RowsTensor()
    t.n = 2 ** 20 + 1
    assert okge_lib.okge_adagrad_rows(t, 1, 0.3, 1e-8, None, 0, None) == -2     # OKGE_ERR_UNSUPPORTED, before anything is read
    t.n = 0
    assert okge_lib.okge_adagrad_rows(t, 1, 0.3, 1e-8, None, 0, None) == 0      # n = 0: a no-op
