"""okge_adam_rows (the sort of okge_adagrad_rows + rows_update_kernel<AdamRows>, csrc/okge_sparse.hip) through HotPath.adam_rows,
against sparse_adam64 of tests/adam_reference.py applied to the host's ascending-position fp32 coalescing (coalesce32), under
adam_caps: row lengths on the 16-byte path and on the single-float path, gradient rows read through a leading dimension, occurrence
counts around the sort's chunk of 1024, one id repeated 3000 times, two tensors in one call.  Rows no id names keep their bits in p
and both moments; a second run from the same inputs gives the same bits; n = 0 leaves the tables alone and still advances t; ids
outside the table are skipped and counted.  Every capped comparison prints `RATIO <case> <tensor> <max error / cap> | <sparse_adam32>`."""
import numpy as np
import pytest
import torch

import adam_reference as A
from open_knowledge_graph_embeddings_amd import _native as N
from open_knowledge_graph_embeddings_amd import hotpath as H

pytestmark = pytest.mark.gpu

LR, BETAS, EPS = 1e-2, (0.9, 0.999), 1e-8
ROW_LENS = (1, 3, 4, 5, 200, 516)
COUNTS = (1, 2, 1024, 1025, 5000)
TABLE = 700


@pytest.fixture(scope="module")
def hp(okge_lib):
    return H.HotPath("cuda:0")


def _bits(x):
    return x.view(torch.int32)


class Table:
    """a table with warm moments at step count t0 and n occurrence rows; g_pad extra columns behind every gradient row (ld_g > row_len)"""

    def __init__(self, rows, row_len, ids, seed, t0=3, g_pad=0):
        n = int(len(ids))
        p, _, m, v = A.sweep_inputs(rows * row_len, seed, True)
        g = A.sweep_inputs(max(n, 1) * row_len, seed + 1000, True)[1][:n * row_len]
        self.rows, self.row_len, self.t = rows, row_len, int(t0)
        self.h = [x.reshape(rows, row_len).copy() for x in (p, m, v)]
        self.ids, self.hg = np.asarray(ids, np.int32), g.reshape(n, row_len)
        self.p, self.m, self.v = (torch.from_numpy(x).cuda() for x in self.h)
        wide = torch.full((n, row_len + g_pad), 777.0, dtype=torch.float32, device="cuda")
        wide[:, :row_len] = torch.from_numpy(self.hg)
        self.wide, self.g = wide, wide[:, :row_len]
        self.d_ids = torch.from_numpy(self.ids).cuda()
        self.state = H.HotPath.adam_state("cuda:0", t0)

    def arg(self):
        return (self.p, self.m, self.v, self.state, self.d_ids, self.g)

    def check(self, case, tensor):
        """after ONE call: t, the named rows against sparse_adam64 of the coalesced gradient, every other row bit-unchanged"""
        self.t += 1
        assert int(self.state[0].item()) == self.t, (case, tensor)
        named, acc, bad = A.coalesce32(self.ids, self.hg, self.rows)
        got = [x.cpu().numpy() for x in (self.p, self.m, self.v)]
        hp_, hm, hv = self.h
        if named.size:
            r = A.sparse_adam64(hp_[named], acc, hm[named], hv[named], self.t, LR, BETAS, EPS)
            assert not A.underflowed(r).any()
            worst = A.cap_ratios([x[named] for x in got], r, hm[named], hv[named], sparse=True)
            yard = A.cap_ratios(A.sparse_adam32(hp_[named], acc, hm[named], hv[named], self.t, LR, BETAS, EPS), r, hm[named], hv[named], sparse=True)
            for name, w, y in zip("pmv", worst, yard):
                print("RATIO %s %s.%s %.3f | %.3f" % (case, tensor, name, w, y))
            assert all(np.isfinite(x).all() for x in got) and max(worst) <= 1.0, (case, tensor, worst)
        rest = np.ones(self.rows, bool)
        rest[named] = False
        for x, h in zip(got, self.h):
            assert np.array_equal(x[rest].view(np.uint32), h[rest].view(np.uint32)), (case, tensor, "a row no id names moved")
        self.h = got
        return bad


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("row_len", ROW_LENS)
def test_rows_update(hp, row_len, n):
    """ids drawn with repeats from the lower 5/7 of the table (the rest must stand still); ld_g = row_len + 3 on the odd-numbered
    cases: the 16-byte path needs ld_g % 4 == 0, so those walk element by element"""
    rng = np.random.default_rng([row_len, n])
    ids = rng.integers(0, 500, n)
    pad = 3 if (ROW_LENS.index(row_len) + COUNTS.index(n)) % 2 else (4 if row_len % 4 == 0 else 0)
    tb = Table(TABLE, row_len, ids, seed=row_len + n, g_pad=pad)
    case = "rows-d%d-n%d-ld%d" % (row_len, n, row_len + pad)
    hp.adam_rows([tb.arg()], LR, BETAS, EPS)
    assert tb.check(case, "t0") == 0
    hp.adam_rows([tb.arg()], LR, BETAS, EPS)                     # a second step, from the kernel's own state
    assert tb.check(case + "-again", "t0") == 0
    assert bool((tb.wide[:, row_len:] == 777.0).all())          # (the columns behind the gradient rows are not the kernel's)


def test_one_id_repeated_3000_times(hp):
    """one lane group sums the whole run, in position order (coalesce32 does the same): three chunks of the sort, merged"""
    rng = np.random.default_rng(77)
    ids = np.full(3300, 41)
    ids[rng.choice(3300, 300, replace=False)] = rng.integers(0, 500, 300)
    tb = Table(TABLE, 200, ids, seed=5)
    hp.adam_rows([tb.arg()], LR, BETAS, EPS)
    assert tb.check("repeat3000-d200", "t0") == 0


def test_two_tensors_share_the_launches(hp):
    """entity- and relation-shaped tensors in one call: different n, row counts, lane counts and step counts"""
    rng = np.random.default_rng(78)
    a = Table(TABLE, 200, rng.integers(0, 500, 1300), seed=6, t0=0)
    b = Table(37, 24, rng.integers(0, 30, 130), seed=7, t0=9, g_pad=4)
    hp.adam_rows([a.arg(), b.arg()], LR, BETAS, EPS)
    assert a.check("two-tensors", "t0") == 0 and b.check("two-tensors", "t1") == 0


def test_same_bits_from_run_to_run(hp):
    rng = np.random.default_rng(79)
    ids = rng.integers(0, 60, 5000)                              # long runs: ~80 occurrences per id
    out = []
    for _ in range(2):
        tb = Table(TABLE, 516, ids, seed=8)
        hp.adam_rows([tb.arg()], LR, BETAS, EPS)
        torch.cuda.synchronize()
        out.append([x.clone() for x in (tb.p, tb.m, tb.v, tb.state)])
    for x, y in zip(*out):
        assert torch.equal(_bits(x) if x.dtype == torch.float32 else x, _bits(y) if y.dtype == torch.float32 else y)


def test_empty_tensor_advances_t_only(hp):
    """n = 0 (alone, and beside a tensor that has rows): the tables keep their bits, t still advances -- SparseAdam.step counts the
    step before it skips an empty gradient"""
    rng = np.random.default_rng(80)
    e = Table(50, 8, np.zeros(0, np.int64), seed=9, t0=4)
    hp.adam_rows([e.arg()], LR, BETAS, EPS)
    assert e.check("empty-alone", "t0") == 0
    f = Table(TABLE, 24, rng.integers(0, 500, 100), seed=10, t0=1)
    hp.adam_rows([e.arg(), f.arg()], LR, BETAS, EPS)
    assert e.check("empty-first", "t0") == 0 and f.check("empty-first", "t1") == 0
    assert int(e.state[0].item()) == 6


def test_out_of_table_ids_are_skipped_and_counted(hp):
    rng = np.random.default_rng(81)
    assert N.id_errors() == 0
    ids = rng.integers(0, 500, 1500)
    ids[[3, 700, 1499]] = (TABLE, -1, 2 ** 31 - 1)
    tb = Table(TABLE, 64, ids, seed=11)
    hp.adam_rows([tb.arg()], LR, BETAS, EPS)
    assert tb.check("bad-ids", "t0") == 3
    assert N.id_errors() == 3                                    # read AND reset: the id-guard fixture expects zero afterwards
