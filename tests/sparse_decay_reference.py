"""NumPy statement of the row-sparse step with deferred weight decay (include/okge.h: okge_rows_catch_up,
okge_adagrad_rows_decay, okge_adagrad_lazy(OKGE_LAZY_FLUSH)), one table at a time.

State: p, state_sum (rows, d) fp32, row_steps (rows,) = optimizer steps each row has seen, T = steps taken.  Every update of a
row -- with a gradient or decay-only -- is the oracle's dense `adagrad_step` on that row, so a row that has seen k steps holds
exactly what k eager dense steps would have left in it, provided the decay-only ones were applied in order and before the row's
next gradient step.  One training step with window W:
  1. catch_up(ids)      every named row with row_steps < T takes its T - row_steps pending decay-only steps
  2. (forward / backward read the named rows: they must hold their eager values here)
  3. update(ids, g)     coalesce (ascending position, sequential fp32: sparse_reference.coalesce), a lagging named row replays
                        first, then adagrad_step WITH the decay term on the named rows; row_steps = T + 1
  4. due_slice(W)       rows with r % W == T % W and row_steps < T + 1 take their decay-only steps up to T + 1;  T += 1
  5. flush()            every row to T
"""
import numpy as np

from oracle import kge_oracle as ko
import sparse_reference as sr


class DeferredTable:
    def __init__(self, p, state_sum, lr, weight_decay, eps):
        self.p, self.s = p, state_sum
        self.row_steps = np.zeros(p.shape[0], np.int32)
        self.T = 0
        self.hp = (lr, weight_decay, eps)

    def _decay_only(self, rows, upto):
        """rows that stand below `upto` take their pending decay-only steps, one dense step of a zero gradient at a time"""
        for r in rows:
            for _ in range(int(upto) - int(self.row_steps[r])):
                pr, sr_ = self.p[r:r + 1], self.s[r:r + 1]                      # (views: the oracle updates in place)
                ko.adagrad_step(pr, np.zeros_like(pr), sr_, *self.hp)
            self.row_steps[r] = max(int(self.row_steps[r]), int(upto))

    def _named(self, ids):
        ids = np.asarray(ids).reshape(-1)
        return np.unique(ids[(ids >= 0) & (ids < self.p.shape[0])])

    def catch_up(self, ids):
        self._decay_only(self._named(ids), self.T)

    def update(self, ids, g):
        dense, touched = sr.coalesce(ids, g, self.p.shape[0])
        rows = np.flatnonzero(touched)
        self._decay_only(rows, self.T)                                          # a lagging row: the caller skipped the catch-up
        pr, sr_ = self.p[rows], self.s[rows]
        ko.adagrad_step(pr, dense[rows], sr_, *self.hp)
        self.p[rows], self.s[rows] = pr, sr_
        self.row_steps[rows] = self.T + 1

    def due_slice(self, window):
        rows = np.arange(self.p.shape[0])
        self._decay_only(rows[rows % window == self.T % window], self.T + 1)
        self.T += 1

    def step(self, ids, g, window):
        self.catch_up(ids)
        self.update(ids, g)
        self.due_slice(window)

    def flush(self):
        self._decay_only(np.arange(self.p.shape[0]), self.T)
