"""okge_rows_catch_up + okge_adagrad_rows_decay + okge_adagrad_lazy(OKGE_LAZY_FLUSH) against the dense okge_adagrad_step2 at the
same weight decay, fed the densified gradient: tables and accumulators BIT FOR BIT after the flush, and the rows a step names bit
for bit right after their catch-up (what the forward would read).

Densifying: tests/sparse_reference.py's coalesce -- per id, ascending position, sequential fp32, the order the kernel is bound
to.  Lists of up to 2 * table_rows occurrences name every id at most twice (two fp32 addends commute, so any densifier would do);
longer lists on these small tables cannot, and there -- as in the case of one id named 64 times in a row -- the NumPy sequential
sum is the statement the kernel is held to.  The update arithmetic is compared kernel against kernel (both correctly rounded, the
same operation order): NumPy has no fused multiply-add for g' = fma(wd, p, g).

Every table lives between two guard rows (and its row_steps between two guard words): an id of -1 or table_rows that slipped
through a bounds check would write there."""
import numpy as np
import pytest
import torch

from open_knowledge_graph_embeddings_amd import _native as N
from open_knowledge_graph_embeddings_amd import hotpath as H
import sparse_reference as sr

ROW_LENS = [4, 200, 256, 264, 512]        # one lane; a partial wave; the prefetch path's limit; the column loop (twice)
TABLE_ROWS = [37, 400]                    # no multiple of a window or of 16
NS = [0, 1, 63, 64, 65, 1024, 1025, 2500]
WINDOWS = [1, 2, 8]
HPARAMS = [(0.3, 1e-10, 1e-8),            # the short sqrt / div sequences (decay_params_ordinary)
           (0.1, 1e-3, 1e-8)]             # weight decay above 2^-10: the generic path
GUARD = 7.0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _ids(rng, rows, n):
    """n occurrences; every id at most twice when the table allows it (n <= 2 * rows, see the module docstring)"""
    k = n // 2
    if k + n % 2 <= rows:
        perm = rng.permutation(rows)
        return rng.permutation(np.concatenate([perm[:k], perm[:k], perm[k:k + n % 2]])).astype(np.int32)
    return rng.integers(0, rows, n).astype(np.int32)


class _Table:
    """the deferred table between guard rows, and the eager dense twin"""

    def __init__(self, rng, rows, row_len, warm):
        p0 = (rng.standard_normal((rows, row_len)) * 0.1).astype(np.float32)
        s0 = rng.uniform(0.01, 1.0, (rows, row_len)).astype(np.float32) if warm else np.zeros((rows, row_len), np.float32)
        pad = np.full((1, row_len), GUARD, np.float32)
        self.pf, self.sf = _dev(np.concatenate([pad, p0, pad])), _dev(np.concatenate([pad, s0, pad]))
        self.p, self.s = self.pf[1:-1], self.sf[1:-1]
        self.stf = torch.zeros(rows + 2, dtype=torch.int32, device="cuda")
        self.stf[0] = self.stf[-1] = -77
        self.steps = self.stf[1:-1]
        self.pd, self.sd = _dev(p0), _dev(s0)
        self.p0, self.rows, self.row_len = p0, rows, row_len
        assert self.p.is_contiguous() and self.p.data_ptr() % 16 == 0 and self.s.data_ptr() % 16 == 0

    def guards_intact(self):
        return (bool((self.pf[[0, -1]] == GUARD).all()) and bool((self.sf[[0, -1]] == GUARD).all())
                and self.stf[0].item() == -77 and self.stf[-1].item() == -77)


def _dense_step(hp, tabs, denses, hpar):
    """okge_adagrad_step2 on the eager twins (one or two tables), gradients kept"""
    lr, wd, eps = hpar
    second = (tabs[1].pd, _dev(denses[1]), tabs[1].sd) if len(tabs) > 1 else tuple(torch.zeros(4, device="cuda") for _ in range(3))
    hp.adagrad2(tabs[0].pd, _dev(denses[0]), tabs[0].sd, *second, lr, wd, eps, zero_grad=False)


def _run(hp, rng, tab, lists, window, hpar, catch_up=True, tag=None):
    """the steps of `lists` on one table; -> (counters, whether some row lagged before the flush)"""
    lr, wd, eps = hpar
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    for ids in lists:
        g = (rng.standard_normal((len(ids), tab.row_len)) * 1e-2).astype(np.float32)
        ids_d, g_d = _dev(ids), _dev(g)
        if catch_up:
            hp.rows_catch_up([(tab.p, tab.s, ids_d, tab.steps)], counters, lr, wd, eps)
            named = _dev(np.unique(ids[(ids >= 0) & (ids < tab.rows)]).astype(np.int64))
            assert _same_bits(tab.p[named], tab.pd[named]) and _same_bits(tab.s[named], tab.sd[named]), tag
        hp.adagrad_rows_decay([(tab.p, tab.s, ids_d, g_d, tab.steps)], counters, window, lr, wd, eps)
        _dense_step(hp, [tab], [sr.coalesce(ids, g, tab.rows)[0]], hpar)
    T = int(counters[0].item())
    assert T == len(lists) and int(counters[1].item()) == 0, tag
    lagged = bool((tab.steps < T).any())
    assert int(tab.steps.max().item()) <= T and int(tab.steps.min().item()) >= T - (window - 1), tag
    hp.adagrad_lazy([(tab.p, tab.s, tab.s, tab.steps)], counters, window, True, lr, wd, eps)
    assert bool((tab.steps == T).all()) and int(counters[0].item()) == T, tag
    assert _same_bits(tab.p, tab.pd) and _same_bits(tab.s, tab.sd), tag
    assert tab.guards_intact(), tag
    return counters, lagged


@pytest.mark.gpu
@pytest.mark.parametrize("row_len", ROW_LENS)
def test_deferred_rows_equal_dense_steps(okge_lib, row_len):
    """every n at this row length; table size, window, hyper-parameters and cold / warm accumulators rotate through the list (and
    start elsewhere for the next row length), 2 W + 3 steps each"""
    hp = H.HotPath("cuda:0")
    k = ROW_LENS.index(row_len)
    rng = np.random.default_rng(100 + k)
    seen = set()
    for j, n in enumerate(NS):
        rows, window = TABLE_ROWS[(j + k) % 2], WINDOWS[(j + k) % 3]
        hpar, warm = HPARAMS[((j + k) // 2) % 2], bool(((j + k) // 4) % 2)
        seen |= {("rows", rows), ("w", window), ("hp", hpar[1]), ("warm", warm)}
        tab = _Table(rng, rows, row_len, warm)
        lists = [_ids(rng, rows, n) for _ in range(2 * window + 3)]
        if n <= 2 * rows:
            assert all(np.bincount(ids, minlength=1).max() <= 2 for ids in lists)
        tag = (row_len, n, rows, window, hpar, warm)
        _, lagged = _run(hp, rng, tab, lists, window, hpar, tag=tag)
        if window > 1 and n <= 65:
            assert lagged, tag                                      # the deferral happened, or the case shows nothing
        never = np.setdiff1d(np.arange(rows), np.concatenate(lists))
        # the decay is real: rows no list named have moved (under warm accumulators the reference's 1e-10 * p lies below half
        # an ulp of both p and the accumulator: such a step returns the bits it was given, in the dense kernel too)
        if never.size and (not warm or hpar[1] > 1e-10):
            assert not np.array_equal(tab.p.cpu().numpy()[never], tab.p0[never]), tag
    assert len(seen) == 2 + 3 + 2 + 2


@pytest.mark.gpu
@pytest.mark.parametrize("hpar", HPARAMS)
def test_one_id_named_by_64_consecutive_occurrences(okge_lib, hpar):
    """64 lanes of four waves claim one lagging row: one owner replays it, and its 64 gradient rows are added in ascending
    position (the NumPy statement's sequential sum is the densified gradient here)"""
    hp = H.HotPath("cuda:0")
    rng = np.random.default_rng(64)
    for row_len, rows in ((200, 37), (512, 400)):
        tab = _Table(rng, rows, row_len, warm=False)
        lists = [_ids(rng, rows - 8, 20) + 8 for _ in range(6)]     # rows 0..7 are named by nobody ...
        crowd = np.concatenate([lists[3][:7], np.full(64, 5, np.int32), lists[3][7:]])
        lists[3] = crowd                                            # ... until step 3 names row 5 (due at T = 5): it owes 3 steps
        assert (crowd[7:71] == 5).all()
        _run(hp, rng, tab, lists, 8, hpar, tag=(row_len, rows))


@pytest.mark.gpu
def test_out_of_range_ids_are_skipped_and_counted(okge_lib):
    hp = H.HotPath("cuda:0")
    rng = np.random.default_rng(9)
    assert N.id_errors() == 0
    for row_len, rows, window in ((4, 37, 2), (264, 400, 8)):
        tab = _Table(rng, rows, row_len, warm=True)
        lists = []
        for _ in range(5):
            ids = _ids(rng, rows, 65)
            ids[3], ids[40] = -1, rows                              # (the NumPy coalescing skips the same two occurrences)
            lists.append(ids)
        _run(hp, rng, tab, lists, window, HPARAMS[0], tag=(row_len, rows))     # bit-equal, guard rows and guard words untouched
        torch.cuda.synchronize()
        assert N.id_errors() == 2 * 5                               # counted once per step (by the sort); read AND reset


@pytest.mark.gpu
@pytest.mark.parametrize("hpar", HPARAMS)
def test_update_without_catch_up_replays_lagging_rows(okge_lib, hpar):
    hp = H.HotPath("cuda:0")
    rng = np.random.default_rng(12)
    for row_len, rows in ((256, 37), (264, 400), (4, 37)):
        tab = _Table(rng, rows, row_len, warm=False)
        lists = [_ids(rng, rows, 9) for _ in range(2 * 8 + 3)]
        # on the host: some step names a row that neither an earlier list nor the rotating sweep has brought to T
        seen_at = np.zeros(rows, np.int64)
        owed = 0
        for t, ids in enumerate(lists):
            owed += int((seen_at[ids] < t).sum())
            seen_at[ids] = t + 1
            seen_at[np.arange(rows) % 8 == t % 8] = t + 1
        assert owed > 0
        _, lagged = _run(hp, rng, tab, lists, 8, hpar, catch_up=False, tag=(row_len, rows))
        assert lagged


@pytest.mark.gpu
def test_two_tensors_one_call_and_strided_gradient_rows(okge_lib):
    """entity- and relation-shaped tensors in the same launches (different n, row counts), one of them with n = 0 in some steps,
    and gradient rows read through a leading dimension"""
    hp = H.HotPath("cuda:0")
    rng = np.random.default_rng(21)
    lr, wd, eps = hpar = HPARAMS[0]
    a, b = _Table(rng, 400, 200, warm=False), _Table(rng, 37, 200, warm=True)
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    for t in range(7):
        ia, ib = _ids(rng, 400, 130), _ids(rng, 37, 0 if t in (2, 5) else 11)
        ga = (rng.standard_normal((130, 200)) * 1e-2).astype(np.float32)
        wide = (rng.standard_normal((len(ib), 208)) * 1e-2).astype(np.float32)
        gb_d = _dev(wide)[:, :200]                                   # ld_g = 208
        ia_d, ib_d = _dev(ia), _dev(ib)
        hp.rows_catch_up([(a.p, a.s, ia_d, a.steps), (b.p, b.s, ib_d, b.steps)], counters, lr, wd, eps)
        hp.adagrad_rows_decay([(a.p, a.s, ia_d, _dev(ga), a.steps), (b.p, b.s, ib_d, gb_d, b.steps)], counters, 4, lr, wd, eps)
        _dense_step(hp, [a, b], [sr.coalesce(ia, ga, 400)[0], sr.coalesce(ib, wide[:, :200], 37)[0]], hpar)
    assert counters.tolist() == [7, 0] and bool((a.steps < 7).any()) and bool((b.steps < 7).any())
    hp.adagrad_lazy([(a.p, a.s, a.s, a.steps), (b.p, b.s, b.s, b.steps)], counters, 4, True, lr, wd, eps)
    for tab in (a, b):
        assert _same_bits(tab.p, tab.pd) and _same_bits(tab.s, tab.sd) and tab.guards_intact()


@pytest.mark.gpu
def test_preconditions_are_refused_before_any_launch(okge_lib):
    hp = H.HotPath("cuda:0")
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    ids = torch.zeros(3, dtype=torch.int32, device="cuda")

    def table(rows, row_len):
        return (torch.ones(rows, row_len, device="cuda"), torch.ones(rows, row_len, device="cuda"),
                torch.zeros(rows, dtype=torch.int32, device="cuda"))
    p, s, st = table(5, 6)                                          # row_len % 4 != 0
    with pytest.raises(N.OkgeError, match="code -2"):
        hp.rows_catch_up([(p, s, ids, st)], counters, 0.3)
    with pytest.raises(N.OkgeError, match="code -2"):
        hp.adagrad_rows_decay([(p, s, ids, torch.ones(3, 6, device="cuda"), st)], counters, 4, 0.3)
    p, s, st = table(5, 8)
    wide = torch.ones(3, 10, device="cuda")                         # ld_g % 4 != 0
    with pytest.raises(N.OkgeError, match="code -2"):
        hp.adagrad_rows_decay([(p, s, ids, wide[:, :8], st)], counters, 4, 0.3)
    with pytest.raises(N.OkgeError, match="code -2"):               # a base that is not 16-byte aligned
        hp.adagrad_rows_decay([(p, s, ids, torch.ones(3 * 8 + 1, device="cuda")[1:].view(3, 8), st)], counters, 4, 0.3)
    with pytest.raises(N.OkgeError, match="code -1"):
        hp.adagrad_rows_decay([(p, s, ids, torch.ones(3, 8, device="cuda"), st)], counters, 0, 0.3)      # window < 1
    torch.cuda.synchronize()
    assert counters.tolist() == [0, 0] and not st.any() and bool((p == 1).all())     # nothing ran
