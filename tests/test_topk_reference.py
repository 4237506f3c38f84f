"""CPU-only: the NumPy restatement of the top-k order (tests/topk_reference.py) on hand-written known answers, and the
associativity that lets tiles, ranges and shards be merged in any cut."""
import numpy as np

import topk_reference as tr

INF = np.float32(np.inf)


def csr(rows):
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.asarray([c for r in rows for c in r], np.int32)
    return ptr, col


def test_survey_vector_with_filter():
    x = np.asarray([[0.5, 0.9, 0.9, 0.2, 0.3, 0.9, 0.7, 5.0]], np.float32)
    fp, fc = csr([[1, 4, 6, 7]])
    s, c, ids = tr.topk_rows(x, 3, fp, fc, first_id=2)
    assert c.tolist() == [[2, 5, 0]]
    assert s.tolist() == [[np.float32(0.9), np.float32(0.9), np.float32(0.5)]]
    assert ids.tolist() == [[4, 7, 2]]


def test_all_equal_row_orders_by_column():
    x = np.full((1, 9), 0.25, np.float32)
    s, c, _ = tr.topk_rows(x, 4)
    assert c.tolist() == [[0, 1, 2, 3]] and (s == 0.25).all()


def test_nan_orders_as_minus_infinity():
    x = np.asarray([[1.0, np.nan, -np.inf, 2.0]], np.float32)
    s, c, _ = tr.topk_rows(x, 6)
    assert c.tolist() == [[3, 0, 1, 2, -1, -1]]                  # NaN (col 1) ties with -inf (col 2): the column decides
    assert np.isnan(s[0, 2]) and s[0, 3] == -INF                # reported as they are
    assert (s[0, 4:] == -INF).all()
    s, c, _ = tr.topk_rows(np.asarray([[np.nan, -5.0]], np.float32), 2)
    assert c.tolist() == [[1, 0]]                                # after every number


def test_fewer_eligible_than_k_is_padded():
    x = np.asarray([[3.0, 1.0, 2.0, 4.0]], np.float32)
    fp, fc = csr([[0, 3]])
    s, c, ids = tr.topk_rows(x, 5, fp, fc, ids=np.asarray([9, 8, 7, 6]))
    assert c.tolist() == [[2, 1, -1, -1, -1]] and ids.tolist() == [[7, 8, -1, -1, -1]]
    assert s.tolist() == [[2.0, 1.0, -INF, -INF, -INF]]


def test_signed_zeros_compare_equal():
    x = np.asarray([[-0.0, 0.0, -0.0, -1.0]], np.float32)
    s, c, _ = tr.topk_rows(x, 3)
    assert c.tolist() == [[0, 1, 2]]
    assert np.signbit(s[0]).tolist() == [True, False, True]     # the scores keep their own bits


def test_global_columns_and_filter_offset():
    x = np.asarray([[1.0, 3.0, 2.0]], np.float32)
    fp, fc = csr([[4, 11]])                                      # 11 is local column 1; 4 belongs to another shard
    s, c, _ = tr.topk_rows(x, 2, fp, fc, col0=10)
    assert c.tolist() == [[12, 10]]


def test_merge_is_associative_over_any_cut():
    rng = np.random.default_rng(3)
    for trial in range(40):
        B, N, k = int(rng.integers(1, 5)), int(rng.integers(1, 90)), int(rng.integers(1, 12))
        x = rng.choice(np.asarray([-0.5, -0.0, 0.0, 0.5, 1.0, np.nan, -np.inf], np.float32), size=(B, N))
        rows = [sorted(rng.choice(N, size=int(rng.integers(0, N + 1)), replace=False).tolist()) for _ in range(B)]
        fp, fc = csr(rows)
        whole = tr.topk_rows(x, k, fp, fc)
        cuts = sorted(set(rng.integers(0, N + 1, size=int(rng.integers(0, 6))).tolist()) | {0, N})
        parts = [tr.topk_rows(x[:, a:b], k, fp, fc, col0=a) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
        order = rng.permutation(len(parts))
        ms, mc = tr.merge_lists(np.stack([parts[i][0] for i in order]), np.stack([parts[i][1] for i in order]))
        tr.assert_same((ms, mc), whole[:2], f"trial {trial}")
        if len(parts) > 2:                                      # ((a + b) + rest) == (a + b + rest)
            a = tr.merge_lists(np.stack([parts[0][0], parts[1][0]]), np.stack([parts[0][1], parts[1][1]]))
            ms, mc = tr.merge_lists(np.stack([a[0]] + [p[0] for p in parts[2:]]), np.stack([a[1]] + [p[1] for p in parts[2:]]))
            tr.assert_same((ms, mc), whole[:2], f"trial {trial} nested")
