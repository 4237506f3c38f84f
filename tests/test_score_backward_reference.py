"""tests/score_backward_reference.py pinned on the CPU: its float64 formulas are what ATen's autograd gives through the
reference's op sequence (oracle/torch_twin.TwinModel.score, torch.nn.functional.embedding with padding_idx=0), its fp32 chain
restatement is a chain and stays inside the classical bound of one, and split_plan gives the documented cuts."""
import numpy as np
import pytest
import torch

import score_backward_reference as R
from oracle import torch_twin


def _inputs(b, n, d, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: (rng.standard_normal(s) * 0.3).astype(np.float32)          # noqa: E731
    return rng.standard_normal((b, n)).astype(np.float32), f(b, d), f(b, d), f(n, d)


@pytest.mark.parametrize("kind,sp", [("complex", True), ("complex", False), ("distmult", True)])
@pytest.mark.parametrize("b,n,d", [(5, 9, 6), (17, 33, 20)])
def test_float64_formulas_are_autograd_through_the_twin(kind, sp, b, n, d):
    G, ent, rel, cand = _inputs(b, n, d, seed=b + d)
    twin = torch_twin.TwinModel(kind, 4, 4, d).double()
    a, r, c = (torch.from_numpy(x).double().requires_grad_() for x in (ent, rel, cand))
    x = twin.score(a, r, c, sp=sp)
    (x * torch.from_numpy(G).double()).sum().backward()
    ref = R.score_backward(kind, sp, G, ent, rel, cand, np.float64)
    np.testing.assert_allclose(ref["q"] @ cand.astype(np.float64).T, x.detach().numpy(), rtol=0, atol=1e-13)
    for name, t in (("d_ent", a), ("d_rel", r), ("d_cand", c)):
        np.testing.assert_allclose(ref[name], t.grad.numpy(), rtol=0, atol=1e-13, err_msg=name)


def test_fp32_fold_rounds_every_product():
    """the fp32 fold is fold_complex's: four products rounded on their own, then one add / subtract"""
    _, ent, rel, _ = _inputs(40, 1, 14, seed=3)
    for sp in (True, False):
        q = R.fold("complex", sp, ent, rel, np.float32)
        assert q.dtype == np.float32
        e1, e2, r1, r2 = ent[:, :7], ent[:, 7:], rel[:, :7], rel[:, 7:]
        a, b, c, dd = (np.float32(1) * (x * y) for x, y in ((e1, r1), (e2, r2), (e2, r1), (e1, r2)))
        want = np.concatenate([a - b, c + dd] if sp else [a + b, c - dd], axis=1)
        assert np.array_equal(q.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(R.fold("distmult", True, ent, rel, np.float32), ent * rel)


def test_chain_is_a_sequential_fp32_accumulate():
    rng = np.random.default_rng(0)
    A, B = rng.standard_normal((3, 37)).astype(np.float32), rng.standard_normal((37, 2)).astype(np.float32)
    want = np.zeros((3, 2), np.float32)
    for i in range(3):
        for j in range(2):
            acc = np.float32(0)
            for k in range(37):
                acc = np.float32(np.float64(acc) + np.float64(A[i, k]) * np.float64(B[k, j]))
            want[i, j] = acc
    assert np.array_equal(R.chain(A, B), want)
    assert np.array_equal(R.chain(np.ascontiguousarray(A.T), B, transpose_a=True), want)


def test_split_plan_matches_the_documented_cuts():
    assert R.split_plan(64, 64, 64) == (1, 64)                       # n <= 64: one split
    assert R.split_plan(16, 257, 16) == (5, 64)                      # capped by the 64-candidate quarters; the last split holds 1
    assert R.split_plan(64, 4096, 64) == (64, 64)                    # capped at 64
    assert R.split_plan(512, 4099, 512) == (16, 272)                 # capped by 1024 / tiles (64 tiles)
    assert R.split_plan(64, 4099, 64) == (52, 80)                    # 64 asked, k_per rounded up to 80: 52 splits, the last holds 19
    assert R.split_plan(512, 14541, 200) == (32, 464)
    assert R.split_plan(9, 298, 16) == (5, 64)                       # the only split count the suite had seen
    for b, n, d in ((1, 1, 1), (130, 1000, 258), (512, 40000, 30), (63, 1000, 62)):
        splits, k_per = R.split_plan(b, n, d)
        assert 1 <= splits <= 64 and k_per % 16 == 0 and (splits - 1) * k_per < n <= splits * k_per
        assert splits * ((b + 63) // 64) * ((d + 63) // 64) <= 1024 and R.workspace_floats(b, d) >= (2 + splits) * b * d


@pytest.mark.parametrize("b,n,d", [(33, 700, 24), (130, 65, 6), (64, 4099, 8)])
def test_fp32_chain_within_the_classical_bound(b, n, d):
    """|chain - float64| <= K 2^-24 sum |g| |c| for both products (K: the contraction length; the split dQ is chains of
    k_per terms and splits - 1 adds, k_per + splits <= n at these shapes), and it is no exact sum either"""
    G, ent, rel, cand = _inputs(b, n, d, seed=n)
    q32 = R.fold("complex", True, ent, rel, np.float32)
    splits, k_per = R.split_plan(b, n, d)
    assert splits == 1 or k_per + splits <= n
    dq, dq64 = R.product_dq(G, cand, np.float32), R.product_dq(G, cand)
    dc, dc64 = R.product_dc(G, q32, np.float32), R.product_dc(G, q32)
    assert dq.dtype == np.float32 and dc.dtype == np.float32
    assert np.all(np.abs(dq - dq64) <= n * R.U * R.abs_product_dq(G, cand))
    assert np.all(np.abs(dc - dc64) <= b * R.U * R.abs_product_dc(G, q32))
    assert np.abs(dq - dq64).max() > 0 and np.abs(dc - dc64).max() > 0
    # and it is the same product as torch's fp32 matmul up to fp32 rounding
    np.testing.assert_allclose(dq, R.torch_matmul32(G, cand), rtol=0, atol=1e-5 * np.abs(dq64).max())


@pytest.mark.parametrize("d", [1, 5])
def test_scatter_rows_is_embedding_backward(d):
    rng = np.random.default_rng(d)
    rows_n, n = 23, 200
    ids = rng.integers(0, rows_n, n)
    ids[:7] = 0
    ids[50:90] = 11                                                        # a long run
    g = rng.standard_normal((n, d)).astype(np.float32)
    W = torch.zeros(rows_n, d, dtype=torch.float64, requires_grad=True)
    (torch.nn.functional.embedding(torch.from_numpy(ids), W, padding_idx=0) * torch.from_numpy(g).double()).sum().backward()
    got, mag, run = R.scatter_rows(g, ids, 0, np.zeros((rows_n, d)), dtype=np.float64)
    np.testing.assert_allclose(got, W.grad.numpy(), rtol=0, atol=1e-13)
    assert np.all(got[0] == 0) and run[0] == 0 and run[11] == 40 + int((ids[:50] == 11).sum() + (ids[90:] == 11).sum())
    np.testing.assert_allclose(mag[1:], np.stack([np.abs(g[ids == i].astype(np.float64)).sum(0) for i in range(1, rows_n)]), atol=1e-12)
    # fp32: the same sums in sorted-position order, added to what the table held
    base = rng.standard_normal((rows_n, d)).astype(np.float32)
    got32 = R.scatter_rows(g, ids, 0, base)[0]
    assert got32.dtype == np.float32 and np.array_equal(got32[0], base[0])
    for i in range(1, rows_n):
        acc = np.zeros(d, np.float32)
        for j in np.flatnonzero(ids == i):
            acc = acc + g[j]
        assert np.array_equal(got32[i], base[i] + acc), i
    # the id-less range form: position i names row first_id + i
    got_r = R.scatter_rows(g[:5], None, 3, base)[0]
    assert np.array_equal(got_r[3:8], base[3:8] + g[:5]) and np.array_equal(got_r[:3], base[:3]) and np.array_equal(got_r[8:], base[8:])
    assert np.array_equal(R.scatter_rows(g[:0], ids[:0], 0, base)[0], base)


def test_encode_rows_is_masked_embedding():
    rng = np.random.default_rng(2)
    table = rng.standard_normal((30, 9)).astype(np.float32)
    ids = rng.integers(0, 30, 50)
    keep = rng.random((50, 9)) >= 0.3
    mult = R.drop_mult(keep, 0.3)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(0.3))
    assert mult.dtype == np.float32 and set(np.unique(mult)) == {np.float32(0), scale}
    want = torch.nn.functional.embedding(torch.from_numpy(ids), torch.from_numpy(table)).numpy() * np.where(keep, scale, np.float32(0))
    assert np.array_equal(R.encode_rows(table, ids, mult=mult), want.astype(np.float32))
    assert np.array_equal(R.encode_rows(table, None, 4, 6), table[4:10])
