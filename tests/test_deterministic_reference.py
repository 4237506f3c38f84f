"""CPU: tests/deterministic_reference.py, the NumPy statement of the deterministic dense gradient, pinned on a case where the
order of the additions decides the answer and held to a float64 sum on random rows."""
import numpy as np

import deterministic_reference as dr


def test_order_decides_the_known_case():
    """1e8, 1, -1e8 for one id: (1e8 + 1) rounds back to 1e8 in fp32, so ascending position gives 0; any order that adds the two
    large rows first gives 1"""
    rows = np.array([[1e8], [1.0], [-1e8]], np.float32)
    out = dr.densify([2, 2, 2], rows, 4)
    assert out.dtype == np.float32 and out.shape == (4, 1)
    assert out[2, 0] == 0.0 and not out[[0, 1, 3]].any()
    assert dr.densify([2, 2, 2], rows[[0, 2, 1]], 4)[2, 0] == 1.0        # the other order, for contrast
    # accumulate form: into + ... in that order.  (3 + 1e8) rounds to 1e8 (the spacing there is 8), + 1 stays, - 1e8 -> 0,
    # where into + (the store form's 0) would be 3; into[1] = 7 is a row nobody names: kept
    into = np.array([[0.0], [7.0], [3.0], [0.0]], np.float32)
    acc = dr.densify([2, 2, 2], rows, 4, into=into)
    assert acc[2, 0] == 0.0 and acc[1, 0] == 7.0 and into[2, 0] == 3.0      # (`into` itself is not modified)
    # ... and where the row's own value survives: 1 first, then the two large rows cancel around it exactly
    into2 = np.array([[0.0], [0.0], [1e8], [0.0]], np.float32)
    assert dr.densify([2, 2], np.array([[-1e8], [1.0]], np.float32), 4, into=into2)[2, 0] == 1.0
    assert dr.densify([2, 2], np.array([[1.0], [-1e8]], np.float32), 4, into=into2)[2, 0] == 0.0


def test_first_row_is_copied_and_bad_ids_are_skipped():
    rows = np.array([[-0.0, 1.0], [5.0, 5.0], [2.0, 3.0], [9.0, 9.0]], np.float32)
    out = dr.densify([1, 7, 0, -1], rows, 3)
    assert np.signbit(out[1, 0]) and out[1, 1] == 1.0                       # stored, not added to +0
    assert np.array_equal(out[0], rows[2]) and not out[2].any()
    assert not np.signbit(dr.densify([1], rows[:1], 3, into=np.zeros((3, 2), np.float32))[1, 0])   # +0 + -0 = +0
    none = np.zeros((0, 2), np.float32)                                                             # n = 0: nothing is written
    assert not dr.densify([], none, 3).any() and np.array_equal(dr.densify([], none, 3, into=rows[:3]), rows[:3])


def test_against_float64_within_the_sequential_rounding_bound():
    """n sequential fp32 additions: |fl(sum) - sum| <= gamma_{n-1} * sum |g_i|, gamma_k = k u / (1 - k u), u = 2^-24 (Higham,
    Accuracy and Stability of Numerical Algorithms, section 4.2); the accumulate form has one addend more"""
    rng = np.random.default_rng(0)
    u = 2.0 ** -24
    for n, table_rows, row_len in ((1, 3, 4), (50, 7, 5), (700, 3, 16), (2000, 1, 3)):
        ids = rng.integers(0, table_rows, n)
        rows = (rng.standard_normal((n, row_len)) * 10.0 ** rng.integers(-3, 3, (n, 1))).astype(np.float32)
        into = rng.standard_normal((table_rows, row_len)).astype(np.float32)
        for start in (None, into):
            got = dr.densify(ids, rows, table_rows, into=start)
            exact = np.zeros((table_rows, row_len)) if start is None else start.astype(np.float64)
            mass = np.abs(exact)
            np.add.at(exact, ids, rows.astype(np.float64))
            np.add.at(mass, ids, np.abs(rows).astype(np.float64))
            k = np.bincount(ids, minlength=table_rows)[:, None] - (1 if start is None else 0)      # additions per table row
            k = np.maximum(k, 0)
            bound = k * u / (1 - k * u) * mass
            assert np.all(np.abs(got.astype(np.float64) - exact) <= bound), (n, start is None)
            untouched = np.setdiff1d(np.arange(table_rows), ids)
            assert np.array_equal(got[untouched], (np.zeros_like(into) if start is None else into)[untouched])
