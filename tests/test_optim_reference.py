"""tests/optim_reference.py pinned on the CPU: the fp32 restatement stays inside the caps the GPU sweep (test_optim_shapes.py)
asserts, the sweep's inputs make a skipped, doubled or misplaced update an error of at least 64 caps, and the float64 formulas
are the oracle's (oracle.kge_oracle.adagrad_step, itself pinned to torch.optim.Adagrad by test_oracle_golden.py)."""
import numpy as np
import pytest

import optim_reference as R
from conftest import golden
from oracle import kge_oracle as ko

LR, EPS = 0.3, 1e-8
N_SELF = 2_000_000


def _accumulator(kind, rng, n):
    if kind == "cold":
        return np.zeros(n, np.float32)
    if kind == "warm":
        return rng.uniform(0.01, 1.0, n).astype(np.float32)
    return (10.0 ** rng.uniform(-20, 0, n)).astype(np.float32)           # spread over 1e-20 .. 1


@pytest.mark.parametrize("wd", [0.0, 1e-10, 1e-3])
@pytest.mark.parametrize("acc", ["cold", "warm", "spread"])
def test_fp32_restatement_stays_inside_its_caps(acc, wd):
    """2 M elements per configuration; |g| spread over 1e-9 .. 1e-1 with a fifth of the gradients zero"""
    rng = np.random.default_rng([7, ("cold", "warm", "spread").index(acc), int(wd * 1e12)])
    n = N_SELF
    p = (0.1 * rng.standard_normal(n)).astype(np.float32)
    g = (10.0 ** rng.uniform(-9, -1, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    g[rng.random(n) < 0.2] = 0.0
    s = _accumulator(acc, rng, n)
    p1, s1, delta = R.adagrad64(p, g, s, LR, wd, EPS)
    ok = ~R.underflowed(s1)                           # the caps assume no underflow: a handful of |p| < 1e-9 with g = 0, cold
    assert (~ok).sum() <= 8, int((~ok).sum())
    p32, s32 = R.adagrad32(p, g, s, LR, wd, EPS)
    rp, rs = R.cap_ratios(p32[ok], s32[ok], p1[ok], s1[ok], delta[ok])
    print("RATIO self-%s-wd%g p %.3f s %.3f (s against 3u: %.3f)" % (acc, wd, rp, rs, rs * 4 / 3))
    assert rp <= 1.0 and rs <= 1.0, (acc, wd, rp, rs)


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("n", [1025, 262_147, 2_000_003])
def test_gradient_cases_are_not_vacuous(n, warm):
    """on the GPU cases' inputs the update is more than 64 caps on at least 99 % of the elements (float64 alone), and with a cold
    accumulator the accumulator's move is more than 64 of its caps on every element: skipping, doubling or misplacing an update
    cannot hide inside the tolerance"""
    p, g, s = R.sweep_inputs(n, 1, warm)
    for wd in (1e-10, 1e-3):
        p1, s1, delta = R.adagrad64(p, g, s, LR, wd, EPS)
        assert not R.underflowed(s1).any()
        cap_p, cap_s = R.adagrad_caps(p1, s1, delta)
        share = float(np.mean(np.abs(delta) > 64 * cap_p))
        print("SHARE n=%d %s wd=%g |delta| > 64 caps on %.4f of the elements" % (n, "warm" if warm else "cold", wd, share))
        assert share >= 0.99, (n, warm, wd, share)
        if not warm:
            gj2 = s1 - np.asarray(s, np.float64)
            assert np.all(gj2 > 64 * cap_s), (n, wd)


def test_decay_only_rows_move_or_stand_still():
    """g = 0.  wd = 1e-3: every element moves by more than 64 caps (cold and warm).  wd = 1e-10 on a warm accumulator: nothing
    moves -- the float64 update is below a quarter of an ulp of p and of s, and the fp32 chain returns the bits it was given
    (there the GPU test asserts unchanged bits)"""
    n = 262_147
    for warm in (False, True):
        p, _, s = R.sweep_inputs(n, 2, warm)
        g = np.zeros(n, np.float32)
        p1, s1, delta = R.adagrad64(p, g, s, LR, 1e-3, EPS)
        assert not R.underflowed(s1).any()
        cap_p, _ = R.adagrad_caps(p1, s1, delta)
        assert np.all(np.abs(delta) > 64 * cap_p), warm
    p, _, s = R.sweep_inputs(n, 2, True)
    p1, s1, delta = R.adagrad64(p, g, s, LR, 1e-10, EPS)
    assert np.all(np.abs(delta) <= 0.25 * R.U * np.abs(p.astype(np.float64)))
    assert np.all(s1 - s.astype(np.float64) <= 0.25 * R.U * s.astype(np.float64))
    p32, s32 = R.adagrad32(p, g, s, LR, 1e-10, EPS)
    assert np.array_equal(p32.view(np.uint32), p.view(np.uint32)) and np.array_equal(s32.view(np.uint32), s.view(np.uint32))


def test_adagrad64_is_the_oracles_step():
    """one g3 golden restart (the second step: a warm accumulator and the reference's own gradient magnitudes): adagrad64
    rounded to fp32 agrees with the oracle's fp32 step within the caps"""
    z = golden("g3_adagrad_complex")
    lr, wd, eps = float(z["opt_lr"]), float(z["opt_weight_decay"]), float(z["opt_eps"])
    E, Rl = z["s0_E"].copy(), z["s0_R"].copy()
    sE, sR = z["s0_sumE"].copy(), z["s0_sumR"].copy()
    out = ko.step_forward_backward(ko.COMPLEX, E, Rl, (z["s1_po_rel"], z["s1_po_obj"]), (z["s1_sp_subj"], z["s1_sp_rel"]),
                                   z["cand"], z["s1_labels"])
    for p, g, s in ((E, out["dE"].astype(np.float32), sE), (Rl, out["dR"].astype(np.float32), sR)):
        p1, s1, delta = R.adagrad64(p, g, s, lr, wd, eps)
        po, so = ko.adagrad_step(p.copy(), g, s.copy(), lr, wd, eps)
        assert po.dtype == np.float32 and so.dtype == np.float32
        cap_p, cap_s = R.adagrad_caps(p1, s1, delta)
        assert np.all(np.abs(po.astype(np.float64) - p1) <= cap_p)
        assert np.all(np.abs(so.astype(np.float64) - s1) <= cap_s)
        assert np.all(np.abs(p1.astype(np.float32).astype(np.float64) - po) <= cap_p)
        assert (np.abs(delta) > 0).mean() > 0.5                          # (the restart does move)


def test_clip_score_and_meter_restatements():
    """small closed-form cases of the other restatements"""
    total, coef = R.clip64(np.array([3.0], np.float32), np.array([4.0], np.float32), 10.0)
    assert total == np.float32(5.0) and coef == np.float32(1.0)
    total, coef = R.clip64(np.array([3.0, 4.0], np.float32), None, 1.0)
    assert total == np.float32(5.0) and coef == np.float32(1.0) / (np.float32(5.0) + np.float32(1e-6)) and coef < 0.2
    assert R.clip64(np.zeros(3, np.float32), None, 1.0) == (np.float32(0.0), np.float32(1.0))
    s, r, o = (np.array([[1.0, 2.0]], np.float32), np.array([[3.0, 5.0]], np.float32), np.array([[7.0, 11.0]], np.float32))
    sc, A = R.score_triples64("complex", s, r, o)        # s1 o1 r1 + s2 o2 r1 + s1 o2 r2 - s2 o1 r2
    assert sc[0] == 1 * 7 * 3 + 2 * 11 * 3 + 1 * 11 * 5 - 2 * 7 * 5 and A[0] == 21 + 66 + 55 + 70
    sc, A = R.score_triples64("distmult", s, -r, o)
    assert sc[0] == -(21 + 110) and A[0] == 21 + 110
    m = R.rank_meters([0, 2, 3, 9, 10, 49, 50, 2 ** 31 + 5])
    assert m[0] == 8 and m[2] == 123 + 2 ** 31 + 5 and m[3:] == [1, 2, 4, 6]
    assert m[1] == pytest.approx(sum(float(np.float32(1.0) / np.float32(x + 1)) for x in [0, 2, 3, 9, 10, 49, 50, 2 ** 31 + 5]), rel=1e-15)
    assert R.rank_meters([]) == [0, 0.0, 0, 0, 0, 0, 0]
